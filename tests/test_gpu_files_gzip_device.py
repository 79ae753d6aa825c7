"""run_files(device_gzip=True) / --gpu-compress: the three .gz files, compressed on the GPU, decode to the bytes of the
plain run's files -- with host-rendered sequences mixed in, through one range and through several -- and the
per-cluster directories of --multiple-files keep the host's gzip."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")
MODES = [(21, True), (17, False)]
IDS = ["canonical", "non_canonical"]


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory):
    from panfeed_amd import synth
    root = tmp_path_factory.mktemp("pg")
    # n_rate: a fifth of the sequences have an 'N' (host-rendered), the others are written by the GPU
    cl = synth.generate(14, 24, first=921, flank=0, mean_len=450, min_len=80, max_len=1000, n_rate=0.2, paralog_rate=0.05)
    names = cl[0].names
    csvp, _gffs, _fas = synth.write_pangenome(str(root), cl)
    return {"csv": csvp, "gffs": str(root / "gffs"), "targets": tuple(names[i] for i in range(0, 24, 2)), "plain": {}}


def _run(pg, out, k, canon, **kw):
    from panfeed_amd.pipeline import run_files
    return run_files(pg["csv"], pg["gffs"], str(out), klength=k, canon=canon, targets=pg["targets"], upstream=40,
                     downstream=30, **kw)


def _plain(pg, tmp_path_factory, k, canon):
    if (k, canon) not in pg["plain"]:
        out = tmp_path_factory.mktemp("plain") / "out"
        st = _run(pg, out, k, canon)
        pg["plain"][(k, canon)] = ({f: (out / f).read_bytes() for f in FILES}, st)
    return pg["plain"][(k, canon)]


def _first_member_bytes(raw):
    d = zlib.decompressobj(31)
    d.decompress(raw)
    return len(raw) - len(d.unused_data)


def _check_gz(out, plain, st):
    assert sorted(os.listdir(out)) == sorted(f + ".gz" for f in FILES)
    behind_headers = 0
    for f in FILES:
        raw = (out / (f + ".gz")).read_bytes()
        assert gzip.decompress(raw) == plain[f], f
        behind_headers += len(raw) - _first_member_bytes(raw)
    # (the statistic is the encoder's own count of each batch's members plus the members the host compressed: it is
    # not derived from the files' sizes)
    assert st["compressed_bytes"] == behind_headers


@pytest.mark.parametrize("k,canon", MODES, ids=IDS)
def test_gz_files_decode_to_the_plain_files(pangenome, tmp_path, tmp_path_factory, k, canon):
    plain, pst = _plain(pangenome, tmp_path_factory, k, canon)
    out = tmp_path / "out"
    st = _run(pangenome, out, k, canon, device_gzip=True)
    _check_gz(out, plain, st)
    assert st["bytes"] == pst["bytes"]
    assert 0 < st["compressed_bytes"] < st["bytes"]


@pytest.mark.parametrize("k,canon", MODES, ids=IDS)
def test_gz_files_through_several_ranges(pangenome, tmp_path, tmp_path_factory, k, canon):
    from panfeed_amd import engine
    plain, pst = _plain(pangenome, tmp_path_factory, k, canon)
    seen = []
    real = engine.Engine.stream_targets_device

    def spy(self, hb, sink, budget=None):
        r = real(self, hb, sink, budget)
        seen.append(r)
        return r
    engine.Engine.stream_targets_device = spy
    try:
        out = tmp_path / "out"
        st = _run(pangenome, out, k, canon, device_gzip=True, targets_text_budget=768 << 10)
    finally:
        engine.Engine.stream_targets_device = real
    kmers_tsv_ranges = max(r[1] for r in seen)
    assert kmers_tsv_ranges > 1
    _check_gz(out, plain, st)
    assert st["bytes"] == pst["bytes"]


class _Crc:
    """a sink's running CRC32 and size of the text handed to it -- as text, or as the gzip members it inflates"""

    def __init__(self):
        self.crc, self.n, self.blocks = 0, 0, 0

    def __call__(self, blk):
        from panfeed_amd.engine import GzipMembers
        self.blocks += 1
        raw = bytes(blk.view) if isinstance(blk, GzipMembers) else None
        if raw is None:
            self.crc, self.n = zlib.crc32(blk, self.crc), self.n + len(blk)
        while raw:
            d = zlib.decompressobj(31)
            text, raw = d.decompress(raw), d.unused_data
            assert d.eof                                     # (every member complete: its CRC32 and ISIZE checked)
            self.crc, self.n = zlib.crc32(text, self.crc), self.n + len(text)


def test_stream_blocks_behind_a_ranges_first():
    """one range of more than two 64 MiB blocks: the blocks behind the first start inside the range's text and use the
    two member buffers alternately; their members must inflate to the plain stream's text"""
    from panfeed_amd import synth
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    samples, k = 1600, 21
    cl = synth.generate(1, samples, first=5000, flank=100, mean_len=1000, min_len=900, max_len=1100, n_rate=0.0)
    stroi = set(cl[0].names)
    hb = build_batch_native([c.record() for c in cl], k, True, samples // 32, stroi=stroi, first_ordinal=0)
    got = {}
    for gz in (False, True):
        eng = Engine(klength=k, max_strains=samples, stroi=stroi, device_gzip=gz)
        sink = _Crc()
        try:
            o = list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=sink))[0]
        finally:
            eng.close()
        assert o.stats["kmers_tsv_ranges"] == 1 and o.stats["kmers_tsv_streamed"] == sink.n
        got[gz] = (sink.crc, sink.n, sink.blocks)
    print("text bytes", got[False][1], "blocks", got[True][2])
    assert got[False][1] > 2 * (64 << 20) and got[True][2] >= 3
    assert got[True][:2] == got[False][:2]


def test_multiple_files_keep_the_host_path(pangenome, tmp_path):
    a, b = tmp_path / "host", tmp_path / "gpu"
    _run(pangenome, a, 21, True, compress=True, multiple_files=True)
    st = _run(pangenome, b, 21, True, device_gzip=True, multiple_files=True)
    assert "compressed_bytes" not in st
    dirs = sorted(os.listdir(a))
    assert dirs and sorted(os.listdir(b)) == dirs
    for d in dirs:
        assert sorted(os.listdir(b / d)) == sorted(f + ".gz" for f in FILES)
        for f in FILES:
            assert gzip.decompress((b / d / (f + ".gz")).read_bytes()) == gzip.decompress((a / d / (f + ".gz")).read_bytes())


def test_command_with_gpu_compress(tmp_path):
    golden = json.load(gzip.open(os.path.join(REPO, "tests", "golden", "cli.json.gz"), "rt"))
    case = next(c for c in golden["cases"] if c["name"] == "targets")
    for rel, text in golden["pangenomes"][case["pangenome"]].items():
        p = os.path.join(tmp_path, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w", newline="") as fh:
            fh.write(text)
    r = subprocess.run([sys.executable, "-m", "panfeed_amd"] + case["args"] + ["-o", "out", "--gpu-compress"], cwd=tmp_path,
                       env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = case["expect"]["outputs"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".gz" for n in exp)
    for name, text in exp.items():
        with gzip.open(tmp_path / "out" / (name + ".gz"), "rt", newline="") as fh:
            assert fh.read() == text, name
