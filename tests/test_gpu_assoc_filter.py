"""The associations filter on the device (downstream.AssocFilter -> pf_assocfilter_*, the af_* kernels of
csrc/pf_rowfilter.hip) against the model of tests/assoc_tables.py, and both downstream tools by the device route against
their own --host-associations route.  No expected text comes from the device route itself."""
import gzip
import io
import json
import math
import os
import sys

import pytest

from conftest import GOLDEN, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
from device_gz_files import member_sizes, write_device_gz  # noqa: E402

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}
RUNS = [(f["case"], i) for f in FIX for i in range(len(f["runs"]))]


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def seeded():
    """the seeded tables and the model's answers, made once: [(text, threshold, Scan)] -- the data lines' seams as they lie
    when the header line is read apart (plain blocks) and when it is scanned along (members)"""
    out = {}
    for skew in (0, len(at.HEADER)):
        text = at.seeded_table(5, skew=skew)
        body = text[len(at.HEADER):]
        assert at.seam_classes(body, skew=skew) >= {(s, p) for s in at.SEAMS for p in at.PARTS}
        out[skew] = (text, 1e-8, at.scan(text, at.PVALUE_FIELD, 1e-8))
    return out


def _device(path, thr, block_bytes=None, device_gunzip=None, n_fields=8):
    """(kept lines, columns(), stats(), the peeled header) of one pass over a file"""
    from panfeed_amd.downstream import AssocFilter
    f = AssocFilter(at.PVALUE_FIELD, n_fields, thr)
    try:
        kept = f.filter_file(str(path), block_bytes=block_bytes, device_gunzip=device_gunzip)
        return kept, f.columns(), f.stats(), f.header
    finally:
        f.close()


def _same(got, m, where, classes=True):
    kept, cols, st, _ = got
    assert kept == m.kept, where
    assert (cols["flags"], cols["rows"], cols["kept"]) == (m.flags, m.rows, m.n_kept), where
    if classes:
        assert cols["classes"] == m.classes, where
    assert st["rows"] == m.rows and st["kept"] == m.n_kept, where
    assert st["device_ms"] > 0 or m.rows == 0, where


@pytest.mark.parametrize("thr", at.THRESHOLDS, ids=[repr(t) for t in at.THRESHOLDS])
def test_case_tables_against_the_model(tmp_path, thr):
    """every case table at every threshold, -t 0, a negative one, inf and nan among them, in blocks of 4 099 bytes and whole
    (at 0.05 in blocks of 64 bytes too): kept lines byte for byte and in order, class bits per column, row flags and counters"""
    for name, text in at.case_tables(thr).items():
        path = tmp_path / f"{name}.tsv"
        path.write_bytes(text)
        m = at.scan(text, at.PVALUE_FIELD, thr)
        for block in (64, 4099, None) if thr == 0.05 else (4099, None):
            got = _device(path, thr, block_bytes=block)
            _same(got, m, (name, block))
            assert got[2]["bytes_scanned"] == len(at.as_scanned(text)), (name, block)
    if math.isnan(thr):        # no row kept: the hand-out is empty (1e-320 is undecided and kept: a table without it)
        path = tmp_path / "int_pvalues.tsv"
        assert _device(path, thr)[0] == b"" and _device(path, thr)[1]["rows"] == 8
    if math.isinf(thr):        # every row kept
        text = at.case_tables(thr)["duplicate_hashes"]
        assert _device(tmp_path / "duplicate_hashes.tsv", thr)[0] == text[len(at.HEADER):]


def test_every_cell_class_on_the_device(tmp_path):
    """each case cell in the p-value column, a row each: whether the row is kept; and each alone in a column: its class bit"""
    cells = [c for bit in at.CLASS_BITS for c in at.CELLS[bit]]
    text = at.HEADER + b"".join(at._row(i, c) + b"\n" for i, c in enumerate(cells))
    path = tmp_path / "cells.tsv"
    path.write_bytes(text)
    m = at.scan(text, at.PVALUE_FIELD, 0.05)
    assert m.classes[at.PVALUE_FIELD] == sum(at.CLASS_BITS)
    _same(_device(path, 0.05), m, "cells")
    # and one cell per column, so that no bit hides in the OR: 300 columns, more than a workgroup gathers in LDS
    wide = (cells * 5)[:300]
    text = b"\t".join(b"c%d" % i for i in range(len(wide))) + b"\n" + b"\t".join(wide) + b"\n"
    path.write_bytes(text)
    m = at.scan(text, at.PVALUE_FIELD, 0.05)
    assert m.classes == [at.classify(c) for c in wide] and m.flags == 0
    _same(_device(path, 0.05, n_fields=len(wide)), m, "one cell a column")


@pytest.mark.parametrize("block", [4099, None])
def test_seeded_table_against_the_model(tmp_path, seeded, block):
    """about 200 KB, three tile ends: a line start, the inside of a p-value cell and a line end on a word, a vector, a
    thread's span and a tile end each"""
    text, thr, m = seeded[0]
    path = tmp_path / "seeded.tsv"
    path.write_bytes(text)
    got = _device(path, thr, block_bytes=block)
    _same(got, m, block)
    assert got[2]["bytes_scanned"] == len(text) - len(at.HEADER) and got[2]["members_inflated"] == 0


def test_members_route(tmp_path, eng, seeded):
    """the same answers through scan_members from a device-gzipped copy: whole in one call, where the header line is scanned
    along and peeled off, and 512 compressed bytes a read, where members straddle reads and lines are carried across calls"""
    from panfeed_amd.downstream import AssocFilter
    text, thr, m = seeded[len(at.HEADER)]
    gz = tmp_path / "seeded.tsv.gz"
    write_device_gz(eng, gz, at.HEADER, text[len(at.HEADER):])
    sizes = member_sizes(gz.read_bytes())
    assert len(sizes) >= 3 and max(sizes) > 2 * 512
    before = (AssocFilter.device_gunzip_files, AssocFilter.fallback_files)
    for block in (None, 512):
        got = _device(gz, thr, block_bytes=block, device_gunzip=True)
        _same(got, m, block)
        assert got[3] == at.HEADER
        assert got[2]["members_inflated"] == len(sizes) and got[2]["text_bytes_inflated"] == len(text)
        assert got[2]["bytes_scanned"] == len(text) - len(at.HEADER)
    assert (AssocFilter.device_gunzip_files, AssocFilter.fallback_files) == (before[0] + 2, before[1])
    # a last line without its newline, and a host-made .gz, which the automatic mode reads through gzip
    cut = at.case_tables()["no_final_newline"]
    write_device_gz(eng, tmp_path / "cut.tsv.gz", at.HEADER, cut[len(at.HEADER):])
    _same(_device(tmp_path / "cut.tsv.gz", 0.05, device_gunzip=True), at.scan(cut, at.PVALUE_FIELD, 0.05), "cut")
    with gzip.open(tmp_path / "host.tsv.gz", "wb") as fh:
        fh.write(text)
    got = _device(tmp_path / "host.tsv.gz", thr)
    _same(got, m, "host gz")
    assert got[2]["members_inflated"] == 0 and got[3] is None


def test_oversized_field_and_line_are_flags(tmp_path):
    """a field of 5 000 bytes and a line of 70 000 set AF_ROW_LONG; the calls return PF_OK and neither row is kept"""
    for name, text in at.long_tables().items():
        path = tmp_path / f"{name}.tsv"
        path.write_bytes(text)
        m = at.scan(text, at.PVALUE_FIELD, 0.05)
        kept, cols, _st, _ = _device(path, 0.05)
        assert cols["flags"] & at.ROW_LONG and m.flags == at.ROW_LONG, name
        assert kept == m.kept and cols["rows"] == m.rows == 3, name
        if name == "field_5000":
            assert cols["flags"] == at.ROW_LONG and cols["classes"] == m.classes


# ------------------------------------------------------------------------------------------------ the tools
def _files(tmp_path, fx):
    exp = CASES[fx["case"]]["expect"]
    paths = {}
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        (tmp_path / name).write_text(exp[name])
        paths[name] = str(tmp_path / name)
    (tmp_path / "assoc.tsv").write_text(fx["associations"])
    return paths, str(tmp_path / "assoc.tsv")


def _run(tool, argv):
    from panfeed_amd import downstream
    out = io.StringIO()
    rc = 0
    try:
        rc = (downstream.get_clusters if tool == "get_clusters" else downstream.get_kmers)(argv, out=out)
    except SystemExit as e:
        rc = int(e.code or 0)
    return out.getvalue(), rc


def _routes():
    from panfeed_amd.downstream import AssocFilter
    return AssocFilter.device_files, AssocFilter.host_files


def _both_routes(tmp_path, tool, argv, want_device=True):
    """the tool's default route against --host-associations: stdout and the -o file; which counters moved"""
    outs = []
    for extra, name in (([], "device.tsv"), (["--host-associations"], "host.tsv")):
        before = _routes()
        po = str(tmp_path / name)
        got, rc = _run(tool, argv + ["-o", po] + extra)
        moved = tuple(b - a for a, b in zip(before, _routes()))
        outs.append((got, rc, open(po, "rb").read() if os.path.exists(po) else None))
        if rc == 0:
            assert moved == ((1, 0) if want_device and not extra else (0, 1)), (extra, moved)
    (got, rc, filtered), (host, rc_host, filtered_host) = outs
    assert rc == rc_host and filtered == filtered_host
    if tool == "get_clusters":
        assert sorted(got.splitlines()) == sorted(host.splitlines())       # (as test_gpu_n4.py compares clusters)
    else:
        assert got == host
    return got, rc


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{i}" for c, i in RUNS])
def test_golden_runs_by_both_routes(tmp_path, case, i):
    fx = next(f for f in FIX if f["case"] == case)
    run = fx["runs"][i]
    paths, pa = _files(tmp_path, fx)
    argv = ["-a", pa, "-p", paths["kmers_to_hashes.tsv"]] + run["args"]
    if run["tool"] == "get_kmers":
        argv += ["-k", paths["kmers.tsv"]]
    got, rc = _both_routes(tmp_path, run["tool"], argv, want_device=run["rc"] == 0)
    assert rc == run["rc"]


def test_a_flagged_table_and_a_missing_column(tmp_path):
    """a CRLF table goes through pandas whole and prints the same; a missing column exits 1 without a device pass"""
    from panfeed_amd.downstream import AssocFilter
    fx = FIX[0]
    paths, pa = _files(tmp_path, fx)
    with open(pa, "rb") as fh:
        text = fh.read()
    with open(pa, "wb") as fh:
        fh.write(text.replace(b"\n", b"\r\n"))
    argv = ["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-t", "0.01"]
    _both_routes(tmp_path, "get_clusters", argv, want_device=False)
    _both_routes(tmp_path, "get_kmers", argv + ["-k", paths["kmers.tsv"]], want_device=False)
    with open(pa, "wb") as fh:
        fh.write(text)
    before, stats = _routes(), AssocFilter.last_stats
    got, rc = _run("get_clusters", argv + ["-c", "no-such-column"])
    assert rc == 1 and got == "" and _routes() == before and AssocFilter.last_stats is stats
