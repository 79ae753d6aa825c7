"""The cases of tests/passing_edges.py held to their own claims and to the oracle, without a GPU: every list keeps
exactly the row indices it was built to keep, every fragment has a hash of its own, the coordinates change their digit
counts where the case says, the conditions of the arena, growth, wrap and content cases hold on the oracle's side, and
the list of seams (EDGES) is covered."""
import collections

import pytest

import kmer_content as kc
import passing_edges as pe

T = pe.KT_ROWS


@pytest.mark.parametrize("geo,k,canon", pe.FRAGMENT_CASES, ids=lambda v: str(v))
def test_every_list_keeps_the_rows_it_claims(geo, k, canon):
    c = pe.fragment_case(geo, k, canon)
    t, g = c.texts, c.geo
    assert len(t.rows) == g.nrows == c.nwin * c.reps and all(h is not None for h in t.row_hash)
    assert len({pe.seq_key(r) for r in t.rows}) == 1, "one target sequence"
    # a hash of its own per fragment, one for everything else
    inside = {}
    for f, (a, b) in g.frags.items():
        assert len({t.row_hash[r] for r in range(a, b)}) == 1, f
        for r in range(a, b):
            assert inside.setdefault(r, f) == f, "fragments overlap"
    hashes = {f: c.hash_of(f) for f in g.frags}
    assert len(set(hashes.values()) | {c.target_hash()}) == len(g.frags) + 1 == len(t.hashes)
    for r, h in enumerate(t.row_hash):
        assert h == (hashes[inside[r]] if r in inside else c.target_hash()), r
    for lst in g.lists:
        kept = t.kept(c.passing(lst))
        assert kept == c.claim(lst), (c.name, lst)
        assert kept and (len(kept) < g.nrows or g.lists[lst][0] == pe.ALL)
        assert t.filter_rows(c.passing(lst)) == [t.rows[i] for i in c.claim(lst)]
    # past two tiles the text allows more than one range at the smallest budget under at least one list (two units and
    # their slack always fit twice the larger one)
    assert (max(pe.ranges_at_smallest_budget(c.units(lst)) for lst in g.lists) > 1) == (g.nrows > 2 * T)


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "both"])
def test_the_claimed_rows_are_the_seams(canon):
    """the row indices of the issue's list, by number"""
    R = 1 if canon else 2
    c = pe.fragment_case("seams", 31 if canon else 32, canon)
    want = dict(row0=list(range(R)), last=list(range(3 * T, 3 * T + R)), r255=list(range(T - R, T)), r256=list(range(T, T + R)),
                r255_256=list(range(T - R, T + R)), r63_64=list(range(64 - R, 64 + R)), wave2=list(range(T + 128, T + 192)))
    for lst, rows in want.items():
        assert c.claim(lst) == rows
    if canon:
        assert (c.claim("row0"), c.claim("r255"), c.claim("r256"), c.claim("r63_64"), c.claim("last")) == \
            ([0], [255], [256], [63, 64], [768])
    units = {lst: c.units(lst) for lst in c.geo.lists}
    assert [bool(u) for u in units["r63_64"]] == [True, False, False, False]            # tiles 1 .. 3 and waves 1 .. 3 empty
    assert [bool(u) for u in units["wave2"]] == [False, True, False, False]
    assert all(r // 64 == (T + 128) // 64 for r in c.claim("wave2")) and len(c.claim("wave2")) == 64
    assert [bool(u) for u in units["across"]] == [True, True, False, True]
    assert [bool(u) for u in units["target"]] == [True, True, False, False]             # tile 2 and the last row are fragments
    assert c.geo.nrows % T == R
    c = pe.fragment_case("tiles", 31 if canon else 32, canon)
    assert [bool(u) for u in c.units("tiles02")] == [True, False, True]
    assert [bool(u) for u in c.units("target")] == [False, True, False]
    assert c.claim("tiles02") == list(range(T)) + list(range(2 * T, 3 * T - R)) and c.geo.nrows % T == T - R
    for k in pe.SWEEP_K:
        c = pe.fragment_case("two", k, canon)
        assert c.claim("seams3") == list(range(T - R, T + R)) + list(range(2 * T - R, 2 * T)) and c.geo.nrows == 2 * T
        assert kc.key_words(k) == {31: 1, 32: 2, 63: 2, 64: 3, 94: 3, 95: 4, 126: 4}[k]


def _field(row, i):
    return int(row.split("\t")[i])


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "both"])
def test_digit_counts_change_at_the_seams(canon):
    R = 1 if canon else 2
    k = 31 if canon else 32
    rows = pe.fragment_case("seams", k, canon).texts.rows
    # forward strand: the first five-digit contig_start is the seam's row (canonical: 255; else the window of rows 256 / 257)
    first = next(i for i, r in enumerate(rows) if _field(r, 5) >= 10_000)
    assert first == (T - 1 if canon else T) and _field(rows[first], 5) == 10_000 and _field(rows[first - 1], 5) == 9_999
    # gene_start goes from negative to positive inside wave 2's kept range
    c = pe.fragment_case("seams", k, canon)
    gs = [_field(rows[i], 7) for i in c.claim("wave2")]
    assert gs[0] < 0 < gs[-1] and 0 in gs
    # digit counts differ on either side of a dropped stretch
    kept = c.claim("across")
    assert len(str(_field(rows[kept[0]], 5))) == 4 and len(str(_field(rows[kept[-1]], 5))) == 5
    assert any(b - a > 64 for a, b in zip(kept, kept[1:]))
    # reverse strand: contig_end drops to four digits there
    c = pe.fragment_case("tiles", k, canon)
    rows = c.texts.rows
    first = next(i for i, r in enumerate(rows) if _field(r, 6) < 10_000)
    assert first == (T - 1 if canon else T) and _field(rows[first], 6) == 9_999 and _field(rows[first - 1], 6) == 10_000
    assert all(_field(r, 4) == -1 for r in rows)
    gs = [_field(rows[i], 7) for i in c.claim("tiles02") if i < T]
    assert gs[0] < 0 < gs[-1]


def test_arena_batch_lists():
    recs, stroi, t, mid = pe.arena_batch()
    by = collections.OrderedDict()
    for i, r in enumerate(t.rows):
        by.setdefault(r.split("\t", 1)[0], []).append(i)
    assert list(by) == [r[1] for r in recs] and list(by)[1] == mid
    assert len({r.split("\t", 2)[1] for r in t.rows}) == 2 == len(stroi)
    second = set(t.kept(t.hashes[::2]))
    assert all(0 < len(second & set(rows)) < len(rows) for rows in by.values()), "every cluster keeps some rows and drops some"
    middle = [h for h in t.hashes if any(idx == mid for (idx, _), h2 in t.pairs.items() if h2 == h)]
    kept = t.kept(middle)
    assert set(by[mid]) <= set(kept) and len(middle) < len(t.hashes)
    # (a pattern is a set of samples: the small clusters' rows of a pattern the middle cluster has too are kept as well)
    assert len(kept) < len(t.rows)


def test_grow_case_has_more_patterns_than_the_pool_and_carries_a_hash_across_batches():
    c = pe.grow_case()
    g, t = pe.GROW_TABLE, c.texts
    passing = pe.grow_passing(c)
    assert (len(t.rows), len(t.kept(t.hashes)), c.n_patterns, len(t.kept(passing))) == (g["rows"], g["listed"], g["patterns"], g["kept"])
    assert c.n_patterns > 512, "the pool of a 1 024-slot pattern table"
    clusters = list(c.by_cluster)
    assert len(clusters) == g["clusters"] and (len(clusters) + pe.GROW_BATCH - 1) // pe.GROW_BATCH > 2
    batches = [clusters[i:i + pe.GROW_BATCH] for i in range(0, len(clusters), pe.GROW_BATCH)]
    assert all(any(c.by_cluster[idx] for idx in b) for b in batches), "every batch has target rows"
    # a passing hash whose pattern first appears in the first batch and whose rows appear in a later one
    first_batch = set(clusters[:pe.GROW_BATCH])
    seen_first = {h for (idx, _), h in t.pairs.items() if idx in first_batch}
    later = {t.row_hash[i] for idx in clusters[pe.GROW_BATCH:] for i in c.by_cluster[idx]}
    # (the first batch's patterns fit the pool: the table grows once ids of an earlier batch are in it)
    assert len(seen_first) + (c.n_patterns - len(t.hashes)) < 512
    carried = set(passing) & seen_first & later
    assert carried, "no passing hash of the first batch has rows later"
    kept = set(t.kept(passing))
    assert all(0 < sum(1 for idx in b for i in c.by_cluster[idx] if i in kept) < sum(len(c.by_cluster[idx]) for idx in b)
               for b in batches), "every batch keeps some rows and drops some"


def test_wrap_index_model():
    w = pe.wrap_index()
    t = w.texts
    kmers = [ln.split("\t")[1] for ln in t.kh.split("\n") if ln and ln.split("\t")[1]]
    assert kmers == w.kmers and len(set(kmers)) == pe.WRAP_NWIN == 511, "place i of the cluster's kept k-mers is row i"
    cap = 64
    while cap < 2 * len(kmers) + 2:
        cap <<= 1
    assert cap == pe.WRAP_CAP, "kt_filter_prepare's size for 511 k-mers"
    assert pe.wraps(w.homes, cap)
    assert 10 in w.absent_wrapping()
    passing, places = w.without(10)
    assert t.kept(passing) == [i for i in range(511) if i not in places] and len(places) == 2
    assert pe._find_wrap_seed(pe.WRAP_SEED + 1)[0] == pe.WRAP_SEED
    # the key layout: one word up to k = 31, the first base in the top bits
    assert pe.key_words_of("C" + "A" * 30) == [1 << 60] and pe.key_words_of("A" * 31 + "C") == [0, 1]
    assert pe.key_words_of("T" + "A" * 31) == [1, 1 << 62]
    assert pe.mix64(0) == 0 and pe.mix64(1) == 0x5692161d100b05e5


def test_wrap_set_model():
    w, s = pe.wrap_index(), pe.wrap_set()
    t = w.texts
    cap = 16
    while cap < 2 * len(s.list) + 2:
        cap <<= 1
    assert cap == pe.SET_CAP and len(set(s.list)) == len(s.list) == 23
    assert s.present in t.hashes and s.absent in t.hashes and s.absent not in s.list
    assert not set(s.fillers) & set(t.hashes)
    homes = s.homes(s.list)
    hp, ha = s.homes([s.present, s.absent])
    # more entries homed in [home, cap - 1] than the run has slots: the chain of `present` and the probe for `absent` wrap
    for h in (hp, ha):
        assert sum(1 for x in homes if x >= h) > cap - h
    assert pe.probe_wraps(ha, pe.occupied(homes, cap))
    assert t.kept(s.list) == t.kept([s.present]) and 0 < len(t.kept(s.list)) < len(t.rows)
    assert t.kept(s.fillers) == []


@pytest.mark.parametrize("k,canon", pe.CONTENT_CASES, ids=lambda v: str(v))
def test_content_list_splits_the_content(k, canon):
    c = pe.content_case(k, canon)
    assert pe.content_conditions(c, c.passing) == []
    assert c.passing[:len(c.passing) - len(c.added)] == c.texts.hashes[0::2] and len(c.added) <= 1
    # the oracle's rows are the model's: the conditions were looked for in the right place
    assert c.texts.rows == [r for m in c.models for r in m.rows]
    assert sum(m.classes[None] for m in c.models) > 0 and sum(n for m in c.models for cl, n in m.classes.items() if cl and cl[0] >= 1) > 0
    assert canon or sum(m.equal_pairs for m in c.models) > 0


def test_every_seam_is_claimed():
    claimed = [e for _, edges in pe.claims() for e in edges]
    assert sorted(set(claimed)) == sorted(set(pe.EDGES)), (set(pe.EDGES) - set(claimed), set(claimed) - set(pe.EDGES))
    assert len({name for name, _ in pe.claims()}) == len(pe.claims())
