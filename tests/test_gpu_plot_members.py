"""panfeed-plot's scan over a .gz of small gzip members (pf_plotgrid_scan_members, csrc/pf_rowfilter.hip; GridBuilder.scan_file
through downstream.route_file): the same grids as from the plain text, both equal to the model of tests/text_tables.py, the
fall-back when the device decoder refuses a file, and panfeed-get-kmers --gz-output -> panfeed-plot end to end."""
import gzip
import io
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_tables as tt  # noqa: E402
from device_gz_files import device_gzip, member_sizes, write_device_gz  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIALS = (float("nan"), -math.inf, -2.5, -0.0, 0.0, 5e-324, 1.5, math.inf)
CHUNK = 32768


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    assert e.L.pf_gzip_device_chunk_bytes() == CHUNK
    yield e
    e.close()


def straddle_text():
    """2 x 32 768 + 1 000 bytes of rows: a row lies across byte 32 768 (where the encoder cuts), another across 65 536, and
    the last one has no newline"""
    rows, n = [], 0
    want = 2 * CHUNK + 1000
    i = 0
    while True:
        row = b"c%d\t%s\t%d\t%s\t%s\tp%d\n" % (i % 7, tt.PLOT_STRAINS[i % 6], i % 13 - 5, (b"ACGT", b"ttag", b"g")[i % 3], (b"1", b"-1")[i % 2], i % 5)
        if n + len(row) + 40 > want:
            break
        rows.append(row)
        n += len(row)
        i += 1
    last = b"tail\ts0\t3\t"
    rows.append(last + b"A" * (want - n - len(last) - len(b"\t1\tp9")) + b"\t1\tp9")
    text = b"".join(rows)
    assert len(text) == want and not text.endswith(b"\n")
    assert b"\n" not in text[CHUNK - 1:CHUNK + 1] and b"\n" not in text[2 * CHUNK - 1:2 * CHUNK + 1]
    return text


TEXTS = {"alignment": tt.plot_alignment_text, "byte_sweep": tt.plot_byte_sweep_text, "straddle": straddle_text}


def _sig_of(text):
    digits = bytes(c for c in text if 48 <= c <= 57)
    return SPECIALS[int(digits or b"0") % len(SPECIALS)]


def _key_of(value):
    from panfeed_amd.plot import _keys
    return 0 if value is None else int(_keys(np.array([value], dtype=np.float64))[0])


def _builder(path, block_bytes=None, device_gunzip=None, strains=tt.PLOT_STRAINS):
    from panfeed_amd.plot import GridBuilder
    gb = GridBuilder([s.decode() for s in strains], tt.PLOT_COLUMNS)
    try:
        gb.scan_file(str(path), block_bytes, device_gunzip)
        gb.finish()
    except BaseException:
        gb.close()
        raise
    return gb


def _snapshot(gb):
    """all a finished builder gives, by cluster name and p-value text (ids are hash order): clusters with min, max, rows and
    the two grids; the texts; lines and records"""
    names = [c.encode() for c in gb.clusters]
    assert len(set(names)) == len(names) and len(set(gb.pvalue_texts)) == len(gb.pvalue_texts)
    gb.set_significance(np.array([_sig_of(t) for t in gb.pvalue_texts], dtype=np.float64))
    ids = [i for i in range(len(names)) if gb.rows[i]]
    grids = dict(zip(ids, gb.grids(ids))) if ids else {}
    clusters = {}
    for i, nm in enumerate(names):
        rows = int(gb.rows[i])
        clusters[nm] = (int(gb.min[i]), int(gb.max[i]), rows, grids[i][0].tobytes(), grids[i][1].tobytes()) if rows else (None, None, 0, b"", b"")
    st = gb.stats()
    return {"clusters": clusters, "texts": sorted(gb.pvalue_texts), "lines": st["lines"], "records": st["records"], "n_records": gb.n_records}


def _model_snapshot(body, strains=tt.PLOT_STRAINS):
    """the same from tests/text_tables.py:plot_model.  A cell of several rows has no one letter: the grids' low words are
    compared only where the model has one row"""
    m = tt.plot_model(tt.as_file(body), tt.PLOT_COLUMNS, strains)
    cells = {}
    for (nm, sid, pos), cell in m.cells.items():
        cells.setdefault(nm, []).append((sid, pos, cell))
    clusters = {}
    for nm, (mn, mx, rows) in m.clusters.items():
        if not rows:
            clusters[nm] = (None, None, 0, None, None)
            continue
        key = np.zeros((len(strains), mx - mn + 1), np.uint64)
        cnt = np.zeros(key.shape, np.uint64)
        for sid, pos, cell in cells[nm]:
            key[sid, pos - mn] = _key_of(tt.ieee_max([_sig_of(t) for t in cell.texts]))
            cnt[sid, pos - mn] = (cell.count << 32) | (cell.letters[0] if cell.count == 1 else 0)
        clusters[nm] = (mn, mx, rows, key, cnt)
    return {"clusters": clusters, "texts": sorted(m.texts), "lines": m.lines, "records": m.records}


def _equals_model(snap, model, n_strains=len(tt.PLOT_STRAINS)):
    assert (snap["texts"], snap["lines"], snap["records"], snap["n_records"]) == (model["texts"], model["lines"], model["records"], model["records"])
    assert set(snap["clusters"]) == set(model["clusters"])
    for nm, (mn, mx, rows, key, cnt) in model["clusters"].items():
        g = snap["clusters"][nm]
        assert g[:3] == (mn, mx, rows), nm
        if rows:
            got_key = np.frombuffer(g[3], np.uint64).reshape(key.shape)
            got_cnt = np.frombuffer(g[4], np.uint64).reshape(key.shape)
            one = (cnt >> np.uint64(32)) == 1
            assert np.array_equal(got_key, key), nm
            assert np.array_equal(got_cnt >> np.uint64(32), cnt >> np.uint64(32)), nm
            assert np.array_equal(got_cnt[one], cnt[one]), nm


@pytest.fixture(scope="module")
def files(tmp_path_factory, eng):
    """per text: its body, the plain file, the device-made .gz, the plain route's snapshot and the model's -- made once"""
    d = tmp_path_factory.mktemp("plot_members")
    out = {}
    for name, make in TEXTS.items():
        body = make()
        plain, gz = d / f"{name}.tsv", d / f"{name}.tsv.gz"
        plain.write_bytes(tt.PLOT_HEADER + body)
        write_device_gz(eng, gz, tt.PLOT_HEADER, body)
        gb = _builder(plain)
        try:
            snap = _snapshot(gb)
        finally:
            gb.close()
        out[name] = {"body": body, "plain": plain, "gz": gz, "snap": snap, "model": _model_snapshot(body)}
    return out


@pytest.mark.parametrize("block_bytes", [1024, None], ids=["reads_of_1024", "one_read"])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_members_give_the_plain_route_s_grids_and_the_model_s(files, name, block_bytes):
    """reads of 1 024 compressed bytes split members between reads and carry lines from call to call"""
    from panfeed_amd.plot import GridBuilder
    f = files[name]
    _equals_model(f["snap"], f["model"])
    n_members = len(member_sizes(f["gz"].read_bytes()))
    before = (GridBuilder.device_gunzip_files, GridBuilder.fallback_files)
    gb = _builder(f["gz"], block_bytes)                      # the automatic route
    try:
        snap = _snapshot(gb)
        st = gb.stats()
    finally:
        gb.close()
    assert snap == f["snap"]
    _equals_model(snap, f["model"])
    assert (GridBuilder.device_gunzip_files, GridBuilder.fallback_files) == (before[0] + 1, before[1])
    assert st["members_inflated"] == n_members and st["text_bytes_inflated"] == len(tt.PLOT_HEADER) + len(f["body"])
    assert st["gunzip_fallbacks"] == 0 and st["inflate_ms"] > 0
    assert st["bytes_scanned"] == len(tt.as_file(f["body"]))
    if name == "straddle":
        assert n_members == 1 + 3 and max(member_sizes(f["gz"].read_bytes())) > 1024


def test_host_gunzip_reads_the_same_file_on_the_host(files):
    from panfeed_amd.plot import GridBuilder
    f = files["straddle"]
    before = (GridBuilder.device_gunzip_files, GridBuilder.fallback_files)
    gb = _builder(f["gz"], None, False)
    try:
        assert _snapshot(gb) == f["snap"] and gb.stats()["members_inflated"] == 0
    finally:
        gb.close()
    assert (GridBuilder.device_gunzip_files, GridBuilder.fallback_files) == before


def test_header_only_file(tmp_path, eng):
    gz = tmp_path / "header.tsv.gz"
    write_device_gz(eng, gz, tt.PLOT_HEADER, b"")
    gb = _builder(gz, None, True)
    try:
        assert gb.clusters == [] and gb.pvalue_texts == [] and gb.n_records == 0
        st = gb.stats()
        assert st["members_inflated"] == 1 and st["lines"] == 0 and st["bytes_scanned"] == 0
    finally:
        gb.close()


def test_a_refused_file_starts_over_on_the_host(tmp_path, files, eng):
    """one gzip.compress member of the whole text has an ISIZE over the decoder's member size: refused at the listing, no
    fault.  Behind members the decoder took, the same refusal comes in a later block: the grid starts over empty"""
    from panfeed_amd.downstream import NotTaken
    from panfeed_amd.plot import GridBuilder
    f = files["straddle"]
    text = tt.PLOT_HEADER + f["body"]
    whole = tmp_path / "whole.tsv.gz"
    whole.write_bytes(gzip.compress(text, mtime=0))
    assert len(text) > 40 << 10 and whole.read_bytes()[:8] == f["gz"].read_bytes()[:8]
    cut = len(tt.PLOT_HEADER) + CHUNK + 777                                  # (inside a row)
    later = tmp_path / "later.tsv.gz"
    later.write_bytes(gzip.compress(tt.PLOT_HEADER, mtime=0) + device_gzip(eng, text[len(tt.PLOT_HEADER):cut]) + gzip.compress(text[cut:], mtime=0))
    assert gzip.decompress(later.read_bytes()) == text and len(text) - cut > CHUNK
    for path, block_bytes in ((whole, None), (later, 4096)):
        before = (GridBuilder.device_gunzip_files, GridBuilder.fallback_files)
        gb = _builder(path, block_bytes)
        try:
            snap, st = _snapshot(gb), gb.stats()
        finally:
            gb.close()
        assert snap == f["snap"], path
        assert (GridBuilder.device_gunzip_files, GridBuilder.fallback_files) == (before[0], before[1] + 1)
        assert st["gunzip_fallbacks"] == 1 and st["members_inflated"] == 0        # (the builder that finished is the fresh one)
        with pytest.raises(NotTaken):
            _builder(path, block_bytes, True)
        assert (GridBuilder.device_gunzip_files, GridBuilder.fallback_files) == (before[0], before[1] + 1)


def test_a_block_that_is_not_taken_leaves_the_grid_as_it_was(files, eng):
    """the library call itself: the grid after the members the decoder took and a refused block is the grid after those
    members alone"""
    import ctypes as C
    from panfeed_amd import _lib
    from panfeed_amd.plot import GridBuilder
    body = tt.plot_alignment_text()
    good = gzip.compress(tt.PLOT_HEADER, mtime=0) + device_gzip(eng, body)
    bad = gzip.compress(b"x\ts0\t1\tA\t1\tp1\n" * 4000, mtime=0)
    gb = GridBuilder([s.decode() for s in tt.PLOT_STRAINS], tt.PLOT_COLUMNS)
    try:
        used, taken = C.c_uint64(), C.c_int()
        _lib.check(gb.L.pf_plotgrid_members_begin(gb.h, 1))
        _lib.check(gb.L.pf_plotgrid_scan_members(gb.h, good, len(good), 1, C.byref(used), C.byref(taken)))
        assert taken.value == 1 and used.value == len(good)
        _lib.check(gb.L.pf_plotgrid_scan_members(gb.h, bad, len(bad), 1, C.byref(used), C.byref(taken)))
        assert taken.value == 0 and used.value == 0 and b"not taken" in gb.L.pf_last_error()
        line, n = C.c_void_p(), C.c_uint64()
        _lib.check(gb.L.pf_plotgrid_members_header(gb.h, C.byref(line), C.byref(n)))
        assert C.string_at(line, n.value) == tt.PLOT_HEADER
        gb.finish()
        _equals_model(_snapshot(gb), files["alignment"]["model"])
    finally:
        gb.close()


# ------------------------------------------------------------------------------------------------ the chain
def test_get_kmers_gz_output_then_plot(tmp_path):
    """a golden case through panfeed-get-kmers --gz-output, then cluster_figures on that file and on the plain stdout text:
    every array of every figure is the same bits, NaN at the same places, and the .gz went the device route"""
    from panfeed_amd import downstream
    from panfeed_amd.plot import GridBuilder, cluster_figures
    with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as fh:
        fx = next(f for f in json.loads(fh.read().decode())["fixtures"] if f["case"] == "rand12_basic")
    exp = next(c for c in all_cases() if c["name"] == "rand12_basic")["expect"]
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        (tmp_path / name).write_text(exp[name])
    (tmp_path / "assoc.tsv").write_text(fx["associations"])
    argv = ["-a", str(tmp_path / "assoc.tsv"), "-p", str(tmp_path / "kmers_to_hashes.tsv"), "-k", str(tmp_path / "kmers.tsv"), "-t", "1"]
    out = io.StringIO()
    assert downstream.get_kmers(argv, out=out) == 0
    plain = out.getvalue()
    assert plain == next(r for r in fx["runs"] if r["tool"] == "get_kmers" and r["args"] == ["-t", "1"])["stdout"]
    gz = tmp_path / "kmers_annotated.tsv.gz"
    assert downstream.get_kmers(argv + ["--gz-output", str(gz)], out=io.StringIO()) == 0
    assert gzip.decompress(gz.read_bytes()).decode() == plain and len(member_sizes(gz.read_bytes())) >= 3
    (tmp_path / "kmers_annotated.tsv").write_text(plain)
    header = plain.split("\n", 1)[0].split("\t")
    strains = sorted({ln.split("\t")[header.index("strain")] for ln in plain.splitlines()[1:]})
    (tmp_path / "pheno.tsv").write_text("strain\tphenotype\n" + "".join(f"{s}\t{i % 2}\n" for i, s in enumerate(strains)))
    kw = dict(threshold=0.01, nucleotides=True, xticks=50)
    before = (GridBuilder.device_gunzip_files, GridBuilder.fallback_files)
    from_gz = list(cluster_figures(str(gz), str(tmp_path / "pheno.tsv"), **kw))
    assert (GridBuilder.device_gunzip_files, GridBuilder.fallback_files) == (before[0] + 1, before[1])
    from_plain = list(cluster_figures(str(tmp_path / "kmers_annotated.tsv"), str(tmp_path / "pheno.tsv"), **kw))
    assert len(from_gz) == len(from_plain) >= 2 and from_gz[0].stats["members_inflated"] >= 3
    for a, b in zip(from_gz, from_plain):
        assert (a.cluster, a.strains, a.hline, a.vline, a.xticks, a.xticklabels, a.titles, a.ylabel) == \
               (b.cluster, b.strains, b.hline, b.vline, b.xticks, b.xticklabels, b.titles, b.ylabel)
        assert np.array_equal(a.positions, b.positions)
        for x, y in ((a.significance, b.significance), (a.nucleotides, b.nucleotides), (a.alpha, b.alpha)):
            x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
            assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))
            assert np.array_equal(np.isnan(x), np.isnan(y))
        assert a.letters.shape == b.letters.shape
        assert [v if isinstance(v, str) else None for v in a.letters.ravel()] == [v if isinstance(v, str) else None for v in b.letters.ravel()]
