"""The row filter over device-gzipped files (RowFilter.filter_file -> pf_rowfilter_scan_members: the members inflated on the
GPU, the text scanned where the inflate left it) and the two downstream tools over such files, against the same filter
over the plain text and against the N4 golden outputs."""
import gzip
import io
import json
import os
import sys

import pytest

from conftest import GOLDEN, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
from device_gz_files import member_sizes, write_device_gz  # noqa: E402

pytestmark = pytest.mark.gpu

HEADERS = {"kmers_to_hashes": b"cluster\tk-mer\thashed_pattern\n",
           "kmers_tsv": b"cluster\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\tgene_start\tgene_end\tstrand\tk-mer\n"}


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def field(line, first_field):
    return line.rstrip(b"\n").split(b"\t")[0 if first_field else -1]


@pytest.fixture(scope="module", params=[0, 1], ids=["last_field", "first_field"])
def table(request, eng, tmp_path_factory):
    """(first_field, plain path, device-gzipped path, keys, plain size, members): rows whose last line has no newline,
    keys of the first row, of the last one, and of the row that lies across the first boundary between two members"""
    first_field = request.param
    C_ = chunk_bytes()
    name = "kmers_tsv" if first_field else "kmers_to_hashes"
    header, rows = HEADERS[name], dc.real_shapes(C_)[name]
    assert not rows.endswith(b"\n") and len(rows) > 4 * C_
    lines = rows.split(b"\n")
    start, end = rows.rfind(b"\n", 0, C_) + 1, rows.find(b"\n", C_)
    assert start < C_ < end
    across = rows[start:end]
    keys = sorted({field(lines[0], first_field), field(lines[-1], first_field), field(across, first_field)})
    d = tmp_path_factory.mktemp(f"gzdev{first_field}")
    plain, gz = d / "t.tsv", d / "t.tsv.gz"
    plain.write_bytes(header + rows)
    write_device_gz(eng, gz, header, rows)
    return first_field, str(plain), str(gz), keys, len(header) + len(rows), member_sizes(gz.read_bytes())


@pytest.fixture(scope="module")
def expected(table):
    from panfeed_amd.downstream import RowFilter
    first_field, plain, _, keys, _, _ = table
    f = RowFilter(keys, first_field=bool(first_field))
    try:
        got = f.filter_file(plain)
    finally:
        f.close()
    rows = got[1].split(b"\n")
    assert got[0] == HEADERS["kmers_tsv" if first_field else "kmers_to_hashes"] and 3 <= len(rows) and got[1].endswith(b"\n")
    return got


@pytest.mark.parametrize("per_call", [1, 2, 3, None])
def test_device_gunzip_equals_the_plain_file(table, expected, per_call):
    """compressed blocks that hold one, two and three whole members a call (the unfinished line is carried on the
    device from call to call), and the default block"""
    from panfeed_amd.downstream import RowFilter
    first_field, _, gz, keys, plain_size, sizes = table
    block = None if per_call is None else per_call * max(sizes) + 1
    f = RowFilter(keys, first_field=bool(first_field))
    try:
        got = f.filter_file(gz, block_bytes=block, device_gunzip=True)
        st = f.stats()
    finally:
        f.close()
    assert got == expected
    # no silent fallback: every member went through the device decoder, and all of the text came from it
    assert st["members_inflated"] == len(sizes) and st["text_bytes_inflated"] == plain_size and st["gunzip_fallbacks"] == 0
    assert st["inflate_ms"] > 0 and 0 < st["inflate_device_bytes"] < 512 << 20


def test_automatic_mode_takes_the_device_route(table, expected):
    from panfeed_amd.downstream import RowFilter
    first_field, _, gz, keys, plain_size, sizes = table
    f = RowFilter(keys, first_field=bool(first_field))
    try:
        assert f.filter_file(gz) == expected
        st = f.stats()
        assert st["gunzip_fallbacks"] == 0 and st["members_inflated"] == len(sizes) and st["text_bytes_inflated"] == plain_size
        assert f.filter_file(gz, device_gunzip=False) == expected
        assert f.stats()["members_inflated"] == len(sizes)
    finally:
        f.close()


def test_files_of_other_writers_go_the_host_way(table, expected, tmp_path):
    """a --compress-made file (zlib's members of 64 KiB of text and more) and one whole-file member of gzip's: the same
    rows, nothing inflated on the device"""
    from panfeed_amd.downstream import NotTaken, RowFilter
    from panfeed_amd.output import ParallelGzipWriter
    first_field, plain, _, keys, _, _ = table
    text = open(plain, "rb").read()
    a, b = tmp_path / "a.tsv.gz", tmp_path / "b.tsv.gz"
    w = ParallelGzipWriter(str(a), chunk_bytes=65536)
    w.write(text.decode())
    w.close()
    b.write_bytes(gzip.compress(text))
    for p in (a, b):
        f = RowFilter(keys, first_field=bool(first_field))
        try:
            assert f.filter_file(str(p)) == expected
            st = f.stats()
            assert st["members_inflated"] == 0 and st["text_bytes_inflated"] == 0 and st["gunzip_fallbacks"] <= 1
            with pytest.raises(NotTaken):
                f.filter_file(str(p), device_gunzip=True)
        finally:
            f.close()


def test_a_damaged_member_raises_what_gzip_raises(table, tmp_path):
    from panfeed_amd.downstream import RowFilter
    first_field, _, gz, keys, _, sizes = table
    raw = bytearray(open(gz, "rb").read())
    raw[sum(sizes[:2]) + sizes[2] // 2] ^= 0x20                  # inside the third member
    p = tmp_path / "damaged.tsv.gz"
    p.write_bytes(bytes(raw))
    f = RowFilter(keys, first_field=bool(first_field))
    try:
        with pytest.raises(Exception) as host:
            f.filter_file(str(p), device_gunzip=False)
        with pytest.raises(Exception) as auto:
            f.filter_file(str(p))
        assert type(auto.value) is type(host.value) and not isinstance(host.value, AssertionError)
        assert f.stats()["gunzip_fallbacks"] == 1
    finally:
        f.close()


# ---- the two tools over the N4 golden inputs, their two files device-gzipped
with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}


def _run(tool, argv):
    from panfeed_amd import downstream
    out = io.StringIO()
    rc = 0
    try:
        rc = (downstream.get_clusters if tool == "get_clusters" else downstream.get_kmers)(argv, out=out)
    except SystemExit as e:
        rc = int(e.code or 0)
    return out.getvalue(), rc


@pytest.mark.parametrize("tool", ["get_clusters", "get_kmers"])
def test_tools_over_device_gzipped_files(eng, tmp_path, tool):
    fx = FIX[0]
    exp = CASES[fx["case"]]["expect"]
    paths = {}
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        text = exp[name].encode()
        cut = text.index(b"\n") + 1
        paths[name] = str(tmp_path / (name + ".gz"))
        write_device_gz(eng, paths[name], text[:cut], text[cut:])
    pa = tmp_path / "assoc.tsv"
    pa.write_text(fx["associations"])
    run = next(r for r in fx["runs"] if r["tool"] == tool and r["args"] == ["-t", "0.01"])
    argv = ["-a", str(pa), "-p", paths["kmers_to_hashes.tsv"], "-t", "0.01"] + (["-k", paths["kmers.tsv"]] if tool == "get_kmers" else [])
    from panfeed_amd.downstream import RowFilter
    before = (RowFilter.device_gunzip_files, RowFilter.fallback_files)
    got, rc = _run(tool, argv)
    assert RowFilter.device_gunzip_files > before[0] and RowFilter.fallback_files == before[1]
    before = RowFilter.device_gunzip_files
    host, rc_host = _run(tool, argv + ["--host-gunzip"])
    assert RowFilter.device_gunzip_files == before
    assert rc == run["rc"] == rc_host and got == host
    if tool == "get_clusters":
        assert sorted(got.splitlines()) == sorted(run["stdout"].splitlines())
    else:
        assert got == run["stdout"]
