"""The life of what the library takes from the HIP runtime (csrc/pf_buf.h: streams, events, page-locked blocks, buffers): a
pf_create that fails part-way leaves nothing that a later context stumbles over; a context closed with a stream of kmers.tsv
ended half way and a stream of pattern rows open, both with work in flight, over and over; the four downstream handles made,
used by both routes and closed, over and over; a device index out of range under each handle's own name."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import assoc_tables as at  # noqa: E402
import join_tables as jt  # noqa: E402
import text_tables as tt  # noqa: E402
from device_gz_files import write_device_gz  # noqa: E402

pytestmark = pytest.mark.gpu

ROUNDS = 16
K = 5


def _records():
    from panfeed_amd import synth
    return [c.record() for c in synth.generate(3, 4)], synth.generate(3, 4)[0].names


def _checksum(**kw):
    """result_checksum() of the batch through a fresh engine"""
    from panfeed_amd.engine import Engine
    eng = Engine(klength=K, max_strains=32, **kw)
    try:
        eng.run(_records()[0])
        return eng.result_checksum()
    finally:
        eng.close()


def test_a_create_that_fails_part_way_leaves_later_contexts_alone():
    """single device allocations capped at 16 KiB: the maf tables (33 words each) fit, the pattern table's 4 096 slots of 8
    bytes do not -- pf_create has made its streams, its events and its first buffers by then"""
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    L = _lib.load()
    before = _checksum(pattern_capacity=4096)
    _lib.check(L.pf_debug_limit_alloc(16 << 10, None))
    try:
        with pytest.raises(_lib.PanfeedHipError) as ei:
            Engine(klength=K, max_strains=32, pattern_capacity=4096)
    finally:
        _lib.check(L.pf_debug_limit_alloc(0, None))
    assert ei.value.status == _lib.ERR_OOM
    assert "hipMalloc(%d)" % (4096 * 8) in str(ei.value)
    assert _checksum(pattern_capacity=4096) == before


def _begin_targets(eng, arr, n, budget):
    total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
    rc = eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, budget, C.byref(total), C.byref(ranges), C.byref(peak))
    return rc, ranges.value


def _next(fn, eng):
    from panfeed_amd import _lib
    ptr, nb = C.c_void_p(), C.c_uint64()
    _lib.check(fn(eng.ctx, C.byref(ptr), C.byref(nb)))
    assert nb.value
    return C.string_at(ptr, nb.value)


def _round_with_work_open(records, stroi):
    """(the first block of the kmers.tsv stream, the first slice of the pattern-row stream) of an engine that is closed with
    the second stream open; the first is ended with ranges of its own still to come"""
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    eng = Engine(klength=K, max_strains=32, stroi=stroi, device_gzip=True)
    try:
        hb = build_batch_native(records, K, True, eng.W, stroi=stroi, first_ordinal=0)
        eng.submit_host_batch(hb)
        with eng._target_records(hb) as (arr, n):       # (the stream reads the records until it ends)
            assert n
            # the smallest budget that works, from the library's own message: a range is then a tile or two
            rc, _ = _begin_targets(eng, arr, n, 4096)
            assert rc == _lib.ERR_ARG
            budget = int(re.search(r"smallest budget that works is (\d+)", eng.L.pf_last_error().decode()).group(1))
            rc, ranges = _begin_targets(eng, arr, n, budget)
            assert rc == 0 and ranges >= 3
            block = _next(eng.L.pf_kmers_tsv_stream_next, eng)
            # one open stream per context: the rows' stream is refused while this one has not reached its end ...
            md5, fs = eng.export_patterns()
            ids = np.ascontiguousarray(np.argsort(fs, kind="stable"), dtype=np.uint32)
            total, slices = C.c_uint64(), C.c_uint32()
            begin = lambda: eng.L.pf_pattern_rows_stream_begin(eng.ctx, ids.ctypes.data_as(C.c_void_p), len(ids), 100,  # noqa: E731
                                                               C.byref(total), C.byref(slices))
            assert begin() == _lib.ERR_STATE
            # ... and setting the gzip mode (as it is) ends it where it stands, two ranges written ahead
            _lib.check(eng.L.pf_set_device_gzip(eng.ctx, 1, 0))
            assert begin() == 0 and slices.value >= 3
            piece = _next(eng.L.pf_pattern_rows_stream_next, eng)
            eng.close()                                 # with slice 1 on its way and the others to come
    finally:
        eng.close()
    return block, piece


def test_contexts_that_go_with_work_open():
    import gzip
    records, names = _records()
    stroi = {names[0], names[2]}
    first = _round_with_work_open(records, stroi)
    # (a tile of kmers.tsv rows; the rows of 4 strains that fit 100 bytes)
    assert gzip.decompress(first[0]).count(b"\n") > 1 and gzip.decompress(first[1]).count(b"\n") == 3
    for r in range(1, ROUNDS):
        assert _round_with_work_open(records, stroi) == first, r


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """two-line tables, each as a plain file and as a .gz of device-made members, with what the models make of them"""
    from panfeed_amd.engine import Engine
    d = tmp_path_factory.mktemp("lifecycle")
    rf_lines = [ln + b"\n" for ln in tt.lines_of(tt.rowfilter_alignment_text()) if ln.count(b"\t") == 2]
    rf_kept = next(ln for ln in rf_lines if tt.filter_rows(ln, tt.RF_KEYS, True))
    rf_other = next(ln for ln in rf_lines if not tt.filter_rows(ln, tt.RF_KEYS, True))
    af_rows = [r + b"\n" for r in at.data_lines(at.case_tables()["spellings"])]
    af_kept = next(r for r in af_rows if at.may_pass(r.split(b"\t")[at.PVALUE_FIELD], 0.05))
    af_other = next(r for r in af_rows if not at.may_pass(r.split(b"\t")[at.PVALUE_FIELD], 0.05))
    plot_rows = [ln + b"\n" for ln in tt.lines_of(tt.plot_alignment_text())
                 if tt.plot_model(ln + b"\n", tt.PLOT_COLUMNS, tt.PLOT_STRAINS).records == 1][:2]
    texts = {"rowfilter": (b"first\tmiddle\tlast\n", rf_kept + rf_other),
             "assoc": (at.HEADER, af_kept + af_other),
             "kmerjoin": (jt.KMERS_HEADER, jt.kmers_row("g", "ACG", 0) + b"\n" + jt.kmers_row("other", "ACG", 1) + b"\n"),
             "plot": (tt.PLOT_HEADER, b"".join(plot_rows))}
    out = {}
    eng = Engine(klength=21, max_strains=32)
    try:
        for name, (header, body) in texts.items():
            assert body.count(b"\n") == 2
            plain, gz = d / f"{name}.tsv", d / f"{name}.tsv.gz"
            plain.write_bytes(header + body)
            write_device_gz(eng, gz, header, body)
            out[name] = {"header": header, "body": body, "plain": str(plain), "gz": str(gz)}
    finally:
        eng.close()
    out["rowfilter"]["want"] = tt.filter_rows(out["rowfilter"]["body"], tt.RF_KEYS, True)
    out["assoc"]["want"] = at.scan(at.HEADER + out["assoc"]["body"], at.PVALUE_FIELD, 0.05)[0]
    out["kmerjoin"]["want"] = jt.join_rows(jt.rows_of(jt.KMERS_HEADER + out["kmerjoin"]["body"]), {b"g"}, {(b"g", b"ACG"): b"t0"}, b"")
    out["plot"]["want"] = tt.plot_model(out["plot"]["body"], tt.PLOT_COLUMNS, tt.PLOT_STRAINS).records
    assert out["rowfilter"]["want"] == rf_kept and out["assoc"]["want"] == af_kept
    assert out["kmerjoin"]["want"].count(b"\n") == 1 and out["plot"]["want"] == 2
    return out


def _handles_round(t):
    """what the four handles, made and closed here, give for their tables by the plain route and by the member route"""
    from panfeed_amd import _lib
    from panfeed_amd.downstream import AssocFilter, KmerJoin, RowFilter
    from panfeed_amd.plot import GridBuilder
    got = {}
    rf = RowFilter(tt.RF_KEYS, first_field=True)
    try:
        got["rowfilter"] = [rf.filter_file(t["rowfilter"][p], device_gunzip=g) for p, g in (("plain", False), ("gz", True))]
    finally:
        rf.close()
    af = AssocFilter(at.PVALUE_FIELD, len(at.HEADER.split(b"\t")), 0.05)
    try:
        got["assoc"] = [af.filter_file(t["assoc"][p], device_gunzip=g) for p, g in (("plain", False), ("gz", True))]
        got["assoc"].append(af.columns()["rows"])
    finally:
        af.close()
    kj = KmerJoin([(b"g", 0)], 1, [(b"g", b"ACG")], [b"t0"], [b"t1.0"], b"")
    try:
        got["kmerjoin"] = []
        for p, g in (("plain", False), ("gz", True)):
            plan = kj.survey_file(t["kmerjoin"][p], device_gunzip=g)
            out = []
            kj.join_file(t["kmerjoin"][p], 0, 0, lambda piece: out.append(bytes(piece)))
            got["kmerjoin"].append((plan[0]["rows"], plan[0]["unmatched"], plan[0]["flags"], b"".join(out)))
            _lib.check(kj.L.pf_kmerjoin_reset_counters(kj.h))
    finally:
        kj.close()
    got["plot"] = []
    for p, g in (("plain", False), ("gz", True)):
        gb = GridBuilder([s.decode() for s in tt.PLOT_STRAINS], tt.PLOT_COLUMNS)
        try:
            gb.scan_file(t["plot"][p], device_gunzip=g)
            gb.finish()
            ids = [i for i in range(len(gb.clusters)) if gb.rows[i]]
            gb.set_significance(np.full(len(gb.pvalue_texts), 0.5))
            grids = [(k.tobytes(), c.tobytes()) for k, c in gb.grids(ids)]
            got["plot"].append((sorted(gb.clusters), sorted(gb.pvalue_texts), gb.n_records, sorted(grids)))
        finally:
            gb.close()
    return got


def test_the_four_downstream_handles_made_and_closed(tables):
    first = _handles_round(tables)
    header = tables["rowfilter"]["header"]
    assert first["rowfilter"] == [(header, tables["rowfilter"]["want"])] * 2
    assert first["assoc"] == [tables["assoc"]["want"]] * 2 + [4]          # (two data lines a pass)
    assert first["kmerjoin"] == [(1, 0, 0, tables["kmerjoin"]["want"])] * 2
    assert first["plot"][0] == first["plot"][1] and first["plot"][0][2] == tables["plot"]["want"]
    for r in range(1, ROUNDS):
        assert _handles_round(tables) == first, r


def test_a_device_out_of_range_is_an_argument_error_under_the_handle_s_own_name():
    from panfeed_amd import _lib
    from panfeed_amd.downstream import AssocFilter, KmerJoin, RowFilter
    from panfeed_amd.plot import GridBuilder
    n = _lib.load().pf_device_count()
    assert n >= 1
    makers = {"pf_rowfilter_create": lambda d: RowFilter([b"a"], True, device=d),
              "pf_assocfilter_create": lambda d: AssocFilter(1, 2, 0.05, device=d),
              "pf_kmerjoin_create": lambda d: KmerJoin([], 0, [], [], [], b"", device=d),
              "pf_plotgrid_create": lambda d: GridBuilder(["s0"], tt.PLOT_COLUMNS, device=d)}
    for name, make in makers.items():
        for device in (n, -1):
            with pytest.raises(_lib.PanfeedHipError) as ei:
                make(device)
            assert ei.value.status == _lib.ERR_ARG and f"{name}: no such device" in str(ei.value), (name, device)
