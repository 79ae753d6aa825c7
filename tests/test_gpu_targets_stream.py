"""kmers.tsv of target strains streamed within a device-memory budget (pf_kmers_tsv_stream_begin / _next,
Engine.stream_targets_device, Engine(targets_text_budget=)): ranges cut at tile and host-sequence boundaries, written by
kt_text_kernel into two buffers used alternately; the bytes are the oracle's and the single-buffer path's."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

BUDGET = 768 << 10


def _pangenome(tmp_path, seed):
    from panfeed_amd import synth
    # n_rate: a fifth of the sequences have an 'N' (host-rendered), the others are written by the GPU
    cl = synth.generate(14, 24, first=seed, flank=0, mean_len=450, min_len=80, max_len=1000, n_rate=0.2,
                        paralog_rate=0.05)
    names = cl[0].names
    csvp, gffs, _fas = synth.write_pangenome(str(tmp_path), cl)
    return cl, names, csvp, gffs


def _oracle_kmers_tsv(csvp, gffs, k, canon, targets, up, down):
    from oracle import input_restatement as ir
    from oracle import oracle as po
    strains, table = ir.load_table(csvp)
    gn = sorted(gffs)
    recs = list(ir.iter_gene_clusters(strains, table, ir.load_genomes(gn, [gffs[n] for n in gn]), up, down, False))
    run = po.OracleRun(klength=k, stroi=set(targets), canon=canon)
    run.feed(recs)
    n_with_n = sum(1 for r in recs for nm, seqs in r[0].items() if nm in targets for s in seqs if "N" in s.sequence.upper())
    n_seqs = sum(1 for r in recs for nm, seqs in r[0].items() if nm in targets for s in seqs)
    return run.texts()[0], n_with_n, n_seqs


def _run(gffdir, csvp, k, canon, targets, up, down, budget, sink):
    from panfeed_amd import native_input as ni
    from panfeed_amd.engine import Engine
    eng = Engine(klength=k, canon=canon, max_strains=32, stroi=set(targets), targets_text_budget=budget)
    try:
        with ni.Pangenome(csvp, gffdir, None, up, down, False, targets=targets) as pg:
            outs = list(eng.run_pangenome(pg, batch_clusters=256, device_text=True, targets_sink=sink))
    finally:
        eng.close()
    return outs


@pytest.mark.parametrize("k,canon", [(21, True), (17, False)], ids=["canonical", "non_canonical"])
def test_streamed_ranges_equal_oracle_and_single_buffer(tmp_path, k, canon):
    cl, names, csvp, gffs = _pangenome(tmp_path, 900 + k)
    targets = tuple(names[i] for i in range(0, 24, 2))
    up, down = 40, 30
    gffdir = str(tmp_path / "gffs")
    ek, n_with_n, n_seqs = _oracle_kmers_tsv(csvp, gffs, k, canon, targets, up, down)
    assert 0 < n_with_n < n_seqs, "the batch must mix device-written and host-rendered sequences"
    assert len(ek) > 4 * BUDGET, "the text must need several ranges"

    got = bytearray()
    outs = _run(gffdir, csvp, k, canon, targets, up, down, BUDGET, lambda blk: got.extend(blk))
    assert len(outs) == 1
    st = outs[0].stats
    assert st["kmers_tsv_ranges"] > 1
    assert 0 < st["kmers_tsv_peak_device_bytes"] <= BUDGET
    assert st["kmers_tsv_streamed"] == len(got)
    assert got.decode() == ek

    # the default budget: one range, the single-buffer path's work; and the single-buffer path itself (no sink)
    one = bytearray()
    outs = _run(gffdir, csvp, k, canon, targets, up, down, 8 << 30, lambda blk: one.extend(blk))
    assert outs[0].stats["kmers_tsv_ranges"] == 1
    assert bytes(one) == bytes(got)
    outs = _run(gffdir, csvp, k, canon, targets, up, down, 8 << 30, None)
    assert bytes(outs[0].kmers_tsv) == bytes(got)


def test_streamed_path_succeeds_where_one_buffer_is_out_of_memory():
    """with single device allocations capped below the batch's text size, pf_render_kmers_tsv_device fails as out of
    memory; the streamed path, at a budget whose halves fit under the cap, writes the same bytes"""
    from oracle import oracle as po
    from panfeed_amd import _lib, synth
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    cl = synth.generate(10, 40, first=4321, flank=20, mean_len=400, min_len=80, max_len=900, n_rate=0.15,
                        paralog_rate=0.05)
    names = cl[0].names
    recs = [c.record() for c in cl]
    stroi = set(names[::3])
    k = 25
    run = po.OracleRun(klength=k, stroi=stroi)
    run.feed(recs)
    ek = run.texts()[0].encode()
    cap = len(ek) // 2
    budget = 2 * (cap // 2)              # each half of the budget is below the cap
    assert budget // 2 < cap < len(ek)
    L = _lib.load()
    eng = Engine(klength=k, max_strains=64, stroi=stroi)
    try:
        hb = build_batch_native(recs, k, True, eng.W, stroi=stroi, first_ordinal=0)
        eng.submit_host_batch(hb)
        _lib.check(L.pf_debug_limit_alloc(cap, None))
        try:
            with pytest.raises(_lib.PanfeedHipError) as ei:
                eng.render_targets_device(hb)
            assert ei.value.status == _lib.ERR_OOM
            got = bytearray()
            n, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=budget)
        finally:
            _lib.check(L.pf_debug_limit_alloc(0, None))
        assert bytes(got) == ek and n == len(ek)
        assert ranges > 1 and peak <= budget
        # the context is still good for the single-buffer path once the cap is gone
        assert bytes(eng.render_targets_device(hb)) == ek
    finally:
        eng.close()


def test_budget_below_one_tile_is_an_argument_error():
    """a budget whose half cannot hold one tile (or one host-rendered sequence): PF_ERR_ARG naming the smallest budget
    that works -- no fault, and the context goes on"""
    import re
    from oracle import oracle as po
    from panfeed_amd import _lib, synth
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    cl = synth.generate(4, 16, first=77, flank=0, mean_len=900, min_len=600, max_len=1200, n_rate=0.0, paralog_rate=0.0)
    recs = [c.record() for c in cl]
    stroi = set(cl[0].names[:5])
    run = po.OracleRun(klength=31, stroi=stroi)
    run.feed(recs)
    ek = run.texts()[0].encode()
    eng = Engine(klength=31, max_strains=32, stroi=stroi)
    try:
        hb = build_batch_native(recs, 31, True, eng.W, stroi=stroi, first_ordinal=0)
        eng.submit_host_batch(hb)
        seen = []
        with pytest.raises(_lib.PanfeedHipError) as ei:
            eng.stream_targets_device(hb, seen.append, budget=4096)
        assert ei.value.status == _lib.ERR_ARG and not seen
        smallest = int(re.search(r"smallest budget that works is (\d+)", str(ei.value)).group(1))
        assert 4096 < smallest < len(ek)
        got = bytearray()
        n, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=smallest)
        assert bytes(got) == ek and ranges > 1 and peak <= smallest
        with pytest.raises(_lib.PanfeedHipError):
            eng.stream_targets_device(hb, seen.append, budget=smallest - 2)
        # a stream left with no begin: next() refuses
        ptr, nb = C.c_void_p(), C.c_uint64()
        assert eng.L.pf_kmers_tsv_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)) == _lib.ERR_STATE
    finally:
        eng.close()


@pytest.mark.parametrize("canon", [True, False], ids=["canonical", "non_canonical"])
def test_unit_order_at_the_seams_of_the_plan(canon):
    """a hand-made batch that fixes the order of the text's units where the plan decides it: sequences with no window
    first, last and between a device unit and a host unit, host-rendered sequences next to each other, a tile seam
    inside a sequence, a one-window sequence, a host-rendered sequence as the last text -- whole text, chunks taken
    twice, one range, ranges at the smallest budget and the host renderer all give the oracle's bytes"""
    import re

    import seam_batch
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    from panfeed_amd.packing import build_batch_native
    k = seam_batch.K
    recs, stroi, ek = seam_batch.build(canon)
    eng = Engine(klength=k, canon=canon, max_strains=32, stroi=stroi)
    try:
        hb = build_batch_native(recs, k, canon, eng.W, stroi=stroi, first_ordinal=0)
        eng.submit_host_batch(hb)
        text = eng.render_targets_device(hb)
        assert bytes(text) == ek
        assert b"".join(bytes(blk) for blk in text.chunks(1000)) == ek
        assert b"".join(bytes(blk) for blk in text.chunks(1000)) == ek
        got = bytearray()
        n, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=8 << 30)
        assert bytes(got) == ek and n == len(ek) and ranges == 1
        with pytest.raises(_lib.PanfeedHipError) as ei:
            eng.stream_targets_device(hb, got.extend, budget=4096)
        assert ei.value.status == _lib.ERR_ARG
        smallest = int(re.search(r"smallest budget that works is (\d+)", str(ei.value)).group(1))
        got = bytearray()
        n, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=smallest)
        assert bytes(got) == ek and n == len(ek)
        assert ranges > 1 and peak <= smallest
        assert eng._render_targets(hb, hb.targets).encode() == ek
    finally:
        eng.close()
