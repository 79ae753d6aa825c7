"""The device-gzip form of a sharded run's files without a GPU: world 2 and 3 under gloo, the CPU oracle standing in for
the engine (tests/sharded_stream_worker.py, mode oracle).  The part writer is given gzip members made by the host model of
the device encoder for the two batch files and plain text for the pattern rows (a source without a stream), rank 0
assembles.  Each assembled `.gz` must read back as the reference's file, and the host model of the device decoder must
take the whole file: the header member, the members compressed on the host and the concatenation across ranks are all
members the decoder lists and accepts.  Also here: `finish_shard`'s choice between a source's stream and its renderer."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import all_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in all_cases()}
FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")


def run_stream_world(mode, world, outdir, spec, options=None, timeout=300, expect_failure=False, grace=30):
    """the ranks of one run as processes, waited for with a timeout.  Once one has failed the others get `grace` seconds to
    end by themselves -- a rank that is told of the failure does -- and whatever still runs then, or when the time is up,
    is ended before anything is asserted.  Returns {rank: stats}, or with expect_failure {rank: (exit status, stdout,
    stderr)}: a rank that had to be ended has a negative status."""
    port = str(32700 + (os.getpid() * 11 + world * 17 + hash((spec, json.dumps(options, sort_keys=True))) % 700) % 2500)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "sharded_stream_worker.py"), mode, str(r),
                               str(world), port, outdir, spec, json.dumps(options or {})],
                              cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    deadline = time.monotonic() + timeout
    while any(p.poll() is None for p in procs):
        if any(p.returncode not in (None, 0) for p in procs):
            deadline = min(deadline, time.monotonic() + grace)
            grace = float("inf")                                   # (counted from the first failure only)
        if time.monotonic() > deadline:
            for p in procs:
                if p.returncode is None:
                    p.kill()
            break
        time.sleep(0.05)                  # (the ranks write a few lines: the pipes do not fill)
    results = {}
    for r, p in enumerate(procs):
        out, err = p.communicate()
        results[r] = (p.returncode, out, err)
    if expect_failure:
        return results
    stats = {}
    for r, (rc, out, err) in results.items():
        assert rc == 0, f"rank {r} failed:\n{out[-2000:]}\n{err[-4000:]}"
        stats[r] = json.loads([x for x in out.splitlines() if x.startswith("STATS ")][-1][6:])
    return stats


def gunzip_host_model(data):
    """(taken, text) of pf_gunzip_host_model: the device decoder's format functions run on the host"""
    from panfeed_amd import _lib
    from panfeed_amd.engine import _mem
    L = _lib.load()
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(L.pf_gunzip_host_model(data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        return taken.value, bytes(_mem(out, n.value))
    finally:
        L.pf_free_text(out)


def check_member_files(out, expect):
    assert sorted(os.listdir(out)) == sorted(f + ".gz" for f in FILES)          # the parts are gone
    for f in FILES:
        path = os.path.join(out, f + ".gz")
        with open(path, "rb") as fh:
            data = fh.read()
        assert gzip.decompress(data).decode() == expect[f], f
        assert subprocess.run(["gzip", "-t", path]).returncode == 0, f
        taken, text = gunzip_host_model(data)
        assert taken == 1, f
        assert text.decode() == expect[f], f
        assert data[:4] == b"\x1f\x8b\x08\x00" and data[4:8] == b"\0\0\0\0", f     # FLG = 0, MTIME = 0: the signature


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["rand12_basic", "rand40_shuffled_missing"])
def test_member_files_equal_reference_files(tmp_path, name, world):
    out = str(tmp_path / "panfeed")
    os.mkdir(out)
    stats = run_stream_world("oracle", world, out, name)
    exp = CASES[name]["expect"]
    check_member_files(out, exp)
    assert stats[0]["patterns"] == exp["n_patterns"] == sum(s["pattern_rows"] for s in stats.values())
    from panfeed_amd.engine import KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, hashes_to_patterns_header
    headers = len(KMERS_TSV_HEADER) + len(KMERS_TO_HASHES_HEADER) + len(hashes_to_patterns_header(CASES[name]["all_strains"]))
    assert sum(s["bytes"] for s in stats.values()) == sum(len(exp[f]) for f in FILES) - headers      # text, not members


def test_an_empty_part_stays_empty(tmp_path):
    """toy_canon at world 3: more ranks than some file has rows for"""
    out = str(tmp_path / "a")
    os.mkdir(out)
    run_stream_world("oracle", 3, out, "toy_canon")
    check_member_files(out, CASES["toy_canon"]["expect"])


def test_a_run_with_no_rows_is_three_valid_files(tmp_path):
    from panfeed_amd.engine import KMERS_TO_HASHES_HEADER, KMERS_TSV_HEADER, hashes_to_patterns_header
    out = str(tmp_path / "none")
    os.mkdir(out)
    run_stream_world("oracle", 2, out, "empty")
    check_member_files(out, {"kmers.tsv": KMERS_TSV_HEADER, "kmers_to_hashes.tsv": KMERS_TO_HASHES_HEADER,
                             "hashes_to_patterns.tsv": hashes_to_patterns_header(["s1", "s2", "s3"])})


def test_host_text_goes_in_as_small_members(tmp_path):
    """text made on the host (a fallback batch, rows without a stream) in a device-gzip part: members of at most the
    device chunk, no first-line member, in order with the GPU's members around it"""
    from panfeed_amd import _lib, sharded
    from panfeed_amd.engine import GzipMembers
    chunk = _lib.load().pf_gzip_device_chunk_bytes()
    w = sharded.ShardWriter(str(tmp_path), 0, device_gzip=True)
    assert w.compress
    line = "cluster\tACGTACGT\thash\n"
    text = line * (3 * chunk // len(line))
    gpu = gzip.compress(b"from the gpu\n", mtime=0)
    w.write_batch("", text)
    w.write_batch("", GzipMembers(memoryview(gpu), 13))
    w.write_batch("", "tail\n")
    w.close()
    assert w.bytes == len(text) + 13 + 5
    with open(tmp_path / ".parts" / "kmers_to_hashes.tsv.gz.part0000", "rb") as fh:
        data = fh.read()
    taken, got = gunzip_host_model(data)
    assert taken == 1 and got.decode() == text + "from the gpu\ntail\n"
    assert os.path.getsize(tmp_path / ".parts" / "kmers.tsv.gz.part0000") == 0


class _Writer:
    def __init__(self):
        self.bytes, self.streamed, self.rendered = 0, [], []

    def sink(self, name):
        assert name == "hashes_to_patterns.tsv"
        return self.streamed.append

    def write_patterns(self, blocks):
        self.rendered += list(blocks)


class _Source:
    def __init__(self):
        self.asked = []

    def export_patterns(self):
        md5 = np.arange(48, dtype=np.uint8).reshape(3, 16)
        return md5, np.array([7, 3, 5], dtype=np.uint64)

    def render_pattern_rows(self, ids):
        self.asked.append(("render", [int(i) for i in ids]))
        yield b"rows"


class _StreamSource(_Source):
    def stream_pattern_rows(self, ids, sink, slice_bytes=0):
        self.asked.append(("stream", [int(i) for i in ids]))
        sink(b"ab")
        sink(b"cde")
        return 5, 5, 2


def test_finish_shard_streams_where_the_source_can():
    from panfeed_amd.sharded import finish_shard
    src, w = _StreamSource(), _Writer()
    assert finish_shard(src, w) == (3, 3)
    assert src.asked == [("stream", [1, 2, 0])]                 # first-seen order
    assert w.streamed == [b"ab", b"cde"] and not w.rendered and w.bytes == 5
    src, w = _Source(), _Writer()
    assert finish_shard(src, w) == (3, 3)
    assert src.asked == [("render", [1, 2, 0])]
    assert w.rendered == [b"rows"] and not w.streamed
