"""The passing-rows filter on the edges of tests/passing_edges.py: rows chosen one by one on the seams of the row
kernels' tiles and waves at the first and last k of every key width, kept k-mers in several arenas, a run in batches
whose pattern table grows, index and set chains that wrap past the last slot (read back from the device through
pf_debug_passing_tables), and palindromes, (AT)n pairs, a reverse-complement pair and a homopolymer under the filter.
The expected text is always the CPU oracle's kmers.tsv filtered by passing_edges.Texts on the oracle's kmers_to_hashes
-- never by the code under test; tests/test_passing_edges.py holds every case to its claims without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import passing_edges as pe

pytestmark = pytest.mark.gpu

EMPTY64 = (1 << 64) - 1


def _engine(k, canon, stroi, max_strains=64, passing=None, **kw):
    from panfeed_amd.engine import Engine
    return Engine(klength=k, canon=canon, max_strains=max_strains, stroi=stroi, maf=0.0, max_items=64, passing_hashes=passing, **kw)


def _submit(eng, recs):
    from panfeed_amd.packing import build_batch_native
    hb = build_batch_native(recs, eng.k, eng.canon, eng.W, stroi=eng.stroi, first_ordinal=eng.next_ordinal)
    eng.next_ordinal += len(recs)
    eng.submit_host_batch(hb)
    return hb


def _smallest_budget(eng, hb):
    """the smallest kmers.tsv budget that works for `hb` under the list in force, as the error for a budget of two bytes
    names it; None where no row is kept (an empty text fits any budget)"""
    from panfeed_amd import _lib
    seen = []
    try:
        eng.stream_targets_device(hb, seen.append, budget=2)
    except _lib.PanfeedHipError as e:
        assert e.status == _lib.ERR_ARG and not seen
        return int(re.search(r"smallest budget that works is (\d+)", str(e)).group(1))
    assert not seen
    return None


def _units(t):
    """the tiles of the text of `t`: every sequence here is written by the device"""
    per_seq = {}
    for r in t.rows:
        key = pe.seq_key(r)
        per_seq[key] = per_seq.get(key, 0) + 1
    return lambda kept: pe.tile_units(t.rows, kept, per_seq)


def _check(eng, hb, t, passing, what, bits=(64,), multi_range=None):
    """every route to the filtered text of the submitted batch under `passing` against the oracle's filtered text: the
    single buffer at each hash width, the sequence ends, the counts, the stream in one range and at the smallest budget
    (with the ranges kt_plan must cut there), the host route"""
    from panfeed_amd import _lib
    kept = t.kept(passing)
    want = pe.text_of(t.rows[i] for i in kept).encode()
    eng.set_passing_hashes(passing)
    for b in tuple(b for b in bits if b != 64) + (64,):
        _lib.check(eng.L.pf_debug_passing_hash_bits(eng.ctx, b))
        got = bytes(eng.render_targets_device(hb))
        stats = eng.passing_stats()
        print(what, "bits", b, "bytes", len(got), "want", len(want), "stats", stats)
        assert got == want, (what, b)
        assert stats[0] == len(set(passing)) and stats[2] == len(t.rows) and stats[3] == len(kept), (what, b, stats)
        if b == 64:
            assert stats[4] == 0
    # pf_kmers_tsv_seq_ends: a sequence none of whose rows are kept repeats the end before it
    n = hb.n_targets
    ends = np.zeros(n, dtype=np.uint64)
    _lib.check(eng.L.pf_kmers_tsv_seq_ends(eng.ctx, ends.ctypes.data, n))
    by_seq = {}
    for i in kept:
        by_seq[pe.seq_key(t.rows[i])] = by_seq.get(pe.seq_key(t.rows[i]), 0) + len(t.rows[i]) + 1
    keys = [(hb.idx[m.cluster], str(m.strain), str(m.seq.id)) for m in hb.targets]
    assert len(set(keys)) == n and set(by_seq) <= set(keys)
    assert ends.tolist() == np.cumsum([by_seq.get(key, 0) for key in keys]).tolist(), what
    # streamed: one range, then the smallest budget the library names
    got = bytearray()
    nb, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=8 << 30)
    assert bytes(got) == want and nb == len(want) and ranges == (1 if want else 0), what
    smallest = _smallest_budget(eng, hb)
    units = _units(t)(kept)
    assert (smallest is None) == (not want)
    if want:
        assert smallest == 2 * (max(units) + 64), (what, smallest, max(units))
        got = bytearray()
        nb, ranges, peak = eng.stream_targets_device(hb, got.extend, budget=smallest)
        print(what, "smallest budget", smallest, "ranges", ranges, "peak", peak)
        assert bytes(got) == want and peak <= smallest, what
        assert ranges == pe.ranges_at_smallest_budget(units), (what, ranges, units)
        if multi_range is not None:
            multi_range.append(ranges)
    # the host route: the host renderer's rows filtered by the engine on the fetched kmers_to_hashes
    out = eng._render(hb, eng.fetch())
    assert out.kmers_tsv.encode() == want, what
    assert (out.stats["kmers_rows_considered"], out.stats["kmers_rows_kept"]) == (len(t.rows), len(kept))
    assert out.kmers_to_hashes == t.kh


# ----------------------------------------------------------------------------------------------- 1. rows chosen one by one
@pytest.mark.parametrize("geo,k,canon", pe.FRAGMENT_CASES, ids=lambda v: str(v))
def test_rows_chosen_one_by_one(geo, k, canon):
    """one engine, one submitted batch, every list of the geometry through set_passing_hashes: the kept rows are the
    claimed indices (held to the oracle by the CPU test), at 64, 4 and 0 hash bits"""
    c = pe.fragment_case(geo, k, canon)
    eng = _engine(k, canon, c.stroi, passing=[])
    try:
        hb = _submit(eng, [c.record])
        ranges = []
        for lst in c.geo.lists:
            assert c.texts.kept(c.passing(lst)) == c.claim(lst)
            _check(eng, hb, c.texts, c.passing(lst), f"{c.name} {lst}", bits=(64, 4, 0), multi_range=ranges)
        assert max(ranges) > 1 or c.geo.nrows <= 2 * pe.KT_ROWS      # (two tiles always fit the smallest budget)
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- 2. several arenas
def _routes(eng, n):
    from panfeed_amd import _lib
    attempts = np.zeros(n, dtype=np.uint32)
    _lib.check(eng.L.pf_debug_cluster_routes(eng.ctx, n, None, None, None, attempts.ctypes.data_as(C.c_void_p)))
    return attempts.tolist()


def test_a_retried_cluster_between_two_small_ones():
    """the middle cluster overflows its scan table and is run again: its kept k-mers live in another arena than its
    neighbours', which stand on either side of it in cl_kmer_off.  kt_filter_prepare's `koff - base`, the kernels'
    arena_key[cluster_arena[c]] and -- rendered while the batch is up -- kh_text_kernel's view of the same arenas."""
    recs, stroi, t, mid = pe.arena_batch()
    eng = _engine(pe.ARENA_K, True, stroi, max_strains=160, passing=[])
    try:
        hb = _submit(eng, recs)
        attempts = _routes(eng, 3)
        print("attempts", attempts, "n_retried", eng.timing()["n_retried"])
        assert attempts[0] == 1 and attempts[1] >= 2 and attempts[2] == 1
        kh, hp = eng.render_device(hb)
        assert bytes(kh).decode() == t.kh and bytes(hp).decode() == t.hp
        middle = [h for h in t.hashes if any(idx == mid and h2 == h for (idx, _), h2 in t.pairs.items())]
        for name, passing in (("every second", t.hashes[::2]), ("the middle cluster's", middle)):
            _check(eng, hb, t, passing, f"arenas, {name}")
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- 3. batches, growing table
def test_batches_with_a_growing_pattern_table():
    """five batches of four clusters through one engine whose pattern table starts with a pool of 512 ids: the table is
    re-made (pattern_rehash_kernel) after the first batch has its ids, later batches' k-mers carry ids of earlier
    ones, and the filter's buffers are reused from text to text"""
    from panfeed_amd import native_input as ni
    c = pe.grow_case()
    t, passing = c.texts, pe.grow_passing(c)
    kept = t.kept(passing)
    assert c.n_patterns > 512
    eng = _engine(pe.GROW_K, True, set(c.targets), pattern_capacity=1024, passing=passing)
    try:
        got, outs, counts = bytearray(), [], []
        with ni.Pangenome(c.csvp, c.gffdir, None, pe.GROW_UP, pe.GROW_DOWN, False, targets=c.targets) as pg:
            for out in eng.run_pangenome(pg, batch_clusters=pe.GROW_BATCH, device_text=True, targets_sink=got.extend):
                outs.append(out.stats)
                counts.append(eng.pattern_count())
        print("batches", len(outs), "patterns after each", counts, "rows", [(s["kmers_rows_considered"], s["kmers_rows_kept"]) for s in outs])
        assert len(outs) > 2
        assert counts[0] < 512 < counts[-1] == c.n_patterns, "the table grew after the first batch's ids were given out"
        assert bytes(got).decode() == pe.text_of(t.rows[i] for i in kept)
        assert sum(s["kmers_rows_considered"] for s in outs) == len(t.rows)
        assert sum(s["kmers_rows_kept"] for s in outs) == len(kept)
        assert all(s["passing_digests"] == len(passing) for s in outs)
        # the filter off on the same engine: a further batch gives the unfiltered text
        eng.set_passing_hashes(None)
        first = list(c.by_cluster)[:pe.GROW_BATCH]
        with ni.Pangenome(c.csvp, c.gffdir, None, pe.GROW_UP, pe.GROW_DOWN, False, targets=c.targets) as pg:
            hb = next(iter(pg.batches(pe.GROW_K, True, eng.W, max_clusters=pe.GROW_BATCH, first_ordinal=eng.next_ordinal)))
            eng.submit_host_batch(hb)
            assert list(hb.idx) == first
            assert bytes(eng.render_targets_device(hb)).decode() == pe.text_of(t.rows[i] for idx in first for i in c.by_cluster[idx])
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- 4. chains that wrap
def _table(eng, which):
    """the whole of one of the filter's device tables: which = 0 -> [slots, 4] (d0, d1, h, used), 1 / 2 -> [slots]"""
    from panfeed_amd import _lib
    slots = C.c_uint64()
    _lib.check(eng.L.pf_debug_passing_tables(eng.ctx, which, 0, 0, None, C.byref(slots)))
    out = np.zeros((slots.value, 4) if which == 0 else slots.value, dtype=np.uint64)
    _lib.check(eng.L.pf_debug_passing_tables(eng.ctx, which, 0, slots.value, out.ctypes.data_as(C.c_void_p), None))
    return out


def test_index_chains_wrap_past_the_last_slot():
    """511 kept k-mers in an index of 1 024 slots.  The device's own table says where every entry is homed: more than t
    entries homed in the top t slots, so an entry sits below its home whatever order the CAS races took, and every
    row's probe -- the wrapped ones included -- found its key.  Then one fragment's hash leaves the list: a probe for
    its keys crosses the table's end to a free slot and the rows go."""
    w = pe.wrap_index()
    t, cap = w.texts, pe.WRAP_CAP
    eng = _engine(w.k, True, w.stroi, passing=t.hashes)
    try:
        hb = _submit(eng, [w.record])
        assert bytes(eng.render_targets_device(hb)).decode() == t.kt
        ref, hsh = _table(eng, 1), _table(eng, 2)
        assert len(ref) == len(hsh) == cap
        used = ref != np.uint64(EMPTY64)
        assert int(used.sum()) == len(w.kmers) == 511
        place_hash = {}
        for slot in np.flatnonzero(used).tolist():
            r = int(ref[slot])
            assert r >> 32 == 0 and (r & 0xFFFFFFFF) < 511
            place_hash[r & 0xFFFFFFFF] = int(hsh[slot])
        assert len(place_hash) == 511
        # the restated pass_key_hash against the device, entry by entry
        assert [place_hash[i] for i in range(511)] == [pe.key_hash(0, km) for km in w.kmers]
        homes = [place_hash[i] & (cap - 1) for i in range(511)]
        top = max(range(1, cap), key=lambda x: sum(1 for h in homes if h >= cap - x) - x)
        print("index: entries homed in the top", top, "slots:", sum(1 for h in homes if h >= cap - top))
        assert pe.wraps(homes, cap), "no chain of this index wraps: pick another seed"
        assert used.tolist() == pe.occupied(homes, cap)
        # one hash less: the probes for its keys wrap to a free slot
        passing, places = w.without(10)
        eng.set_passing_hashes(passing)
        assert bytes(eng.render_targets_device(hb)).decode() == t.filtered(passing)
        assert eng.passing_stats()[1:4] == (511 - len(places), 511, 511 - len(places))
        used = (_table(eng, 1) != np.uint64(EMPTY64)).tolist()
        assert sum(used) == 511 - len(places)
        assert any(pe.probe_wraps(homes[i], used) and not all(used) for i in places), "no probe for an absent key wraps"
    finally:
        eng.close()


def test_set_chains_wrap_and_the_counter_without_a_hash_model():
    from panfeed_amd import _lib
    w, s = pe.wrap_index(), pe.wrap_set()
    t, cap = w.texts, pe.SET_CAP
    eng = _engine(w.k, True, w.stroi, passing=s.list)
    try:
        hb = _submit(eng, [w.record])
        slots = _table(eng, 0)
        assert slots.shape == (cap, 4)
        used = slots[:, 3] != 0
        assert int(used.sum()) == len(s.list)
        by_digest = {(int(d0), int(d1)): int(h) for d0, d1, h, u in slots.tolist() if u}
        # the restated pass_digest_hash against the table the library built
        assert by_digest == {pe.digest_words(h): pe.digest_hash(h) for h in s.list}
        homes = [h & (cap - 1) for h in by_digest.values()]
        hp = by_digest[pe.digest_words(s.present)] & (cap - 1)
        assert sum(1 for x in homes if x >= hp) > cap - hp, "the chain of the present hash does not wrap"
        ha = pe.digest_hash(s.absent) & (cap - 1)
        assert pe.probe_wraps(ha, used.tolist()) and not used.all(), "the probe for the absent hash does not wrap"
        assert bytes(eng.render_targets_device(hb)).decode() == t.filtered(s.list)
        stats = eng.passing_stats()
        assert stats[1] == stats[3] == len(t.kept([s.present])) > 0 and stats[4] == 0
        # fillers only: no row passes, the index stays empty, no comparison is made at 64 bits ...
        eng.set_passing_hashes(s.fillers)
        assert bytes(eng.render_targets_device(hb)) == b""
        stats = eng.passing_stats()
        assert stats[:5] == (len(s.fillers), 0, len(t.rows), 0, 0)
        assert (_table(eng, 1) == np.uint64(EMPTY64)).all()
        # ... and at 0 bits every marked k-mer's probe walks the whole chain of the set and finds nothing
        _lib.check(eng.L.pf_debug_passing_hash_bits(eng.ctx, 0))
        assert bytes(eng.render_targets_device(hb)) == b""
        stats = eng.passing_stats()
        assert stats[:5] == (len(s.fillers), 0, len(t.rows), 0, len(w.kmers) * len(s.fillers))
        _lib.check(eng.L.pf_debug_passing_hash_bits(eng.ctx, 64))
    finally:
        eng.close()


def test_table_hook_refuses_what_it_cannot_answer():
    """PF_ERR_STATE with the filter off, and for the index with no filtered text since the batch, the list or the hash
    width changed; PF_ERR_ARG outside the table; the set may be read as soon as there is a list"""
    from panfeed_amd import _lib
    w = pe.wrap_index()
    eng = _engine(w.k, True, w.stroi)
    try:
        buf = np.zeros(8, dtype=np.uint64)
        slots = C.c_uint64()
        read = lambda which, first, n: eng.L.pf_debug_passing_tables(eng.ctx, which, first, n, buf.ctypes.data_as(C.c_void_p), C.byref(slots))  # noqa: E731
        assert read(0, 0, 1) == _lib.ERR_STATE
        eng.set_passing_hashes(w.texts.hashes[:3])
        assert read(0, 0, 1) == 0 and slots.value == 16
        assert read(1, 0, 1) == _lib.ERR_STATE and read(3, 0, 1) == _lib.ERR_ARG and read(-1, 0, 1) == _lib.ERR_ARG
        hb = _submit(eng, [w.record])
        assert read(2, 0, 1) == _lib.ERR_STATE
        eng.render_targets_device(hb)
        assert read(1, 1023, 1) == 0 and slots.value == 1024 and read(2, 1024, 0) == 0
        assert read(1, 1024, 1) == _lib.ERR_ARG and read(2, 1020, 8) == _lib.ERR_ARG and read(0, 15, 2) == _lib.ERR_ARG
        eng.set_passing_hashes(w.texts.hashes[:2])
        assert read(1, 0, 1) == _lib.ERR_STATE
        eng.set_passing_hashes(None)
        assert read(0, 0, 1) == _lib.ERR_STATE
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------------- 5. content
@pytest.mark.parametrize("k,canon", pe.CONTENT_CASES, ids=lambda v: str(v))
def test_content_under_the_filter(k, canon):
    """kt_row_passes rebuilds the key from the packed bases of the strand that is printed: exact palindromes (a tie),
    near-palindromes decided in the second key word, (AT)n whose two rows print one k-mer, a sequence beside its reverse
    complement, and a homopolymer whose 256 rows probe one slot -- some kept, some dropped, as the CPU test holds"""
    c = pe.content_case(k, canon)
    assert pe.content_conditions(c, c.passing) == []
    eng = _engine(k, canon, c.stroi, passing=[])
    try:
        hb = _submit(eng, c.recs)
        ranges = []
        _check(eng, hb, c.texts, c.passing, f"content k={k} canon={canon}", multi_range=ranges)
        assert ranges[0] > 1
    finally:
        eng.close()
