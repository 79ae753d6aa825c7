"""The case lists of tests/weak_hash_cases.py contain what tests/test_gpu_weak_hash.py relies on.  No GPU, no library."""
import numpy as np

import weak_hash_cases as wc


def _by_name(case):
    return {r[1]: r for r in case["recs"]}


def test_small_cases_hold_every_family():
    for k in wc.SMALL_K:
        case = wc.small_case(k)
        recs = _by_name(case)
        Ds = sorted(wc.n_distinct(r) for n, r in recs.items() if n.startswith("rnd"))
        assert Ds.count(2) == 8 and sum(d >= 20 for d in Ds) >= 3 and min(Ds) == 2 and max(Ds) == 40
        for name in ("tail_edge", "tail_halo"):
            X, X1, X4, X33, Xm = list(dict.fromkeys(wc.sequences(recs[name])))
            assert X.endswith(b"CA") and X1 == X + b"A" and X4 == X + b"AAAA" and X33 == X + b"A" * 33 and Xm == X[:-1]
            assert (len(X) + 31) // 32 == (len(X4) + 31) // 32 or name == "tail_edge" or k % 32 > 28   # the same packed words
        a, b, c = list(dict.fromkeys(wc.sequences(recs["last_base"])))
        assert len(a) % 32 == 0 and a[:-1] == b[:-1] == c[:-1] and len({a[-1], b[-1], c[-1]}) == 3
        w0 = list(dict.fromkeys(wc.sequences(recs["word0"])))
        assert all(s[32:] == w0[0][32:] and s[:32] != w0[0][:32] for s in w0[1:])
        assert wc.n_distinct(recs["copies_a"]) == wc.n_distinct(recs["copies_b"]) == 1
        assert not wc.eligible(recs["three"]) and all(wc.eligible(r) for n, r in recs.items() if n != "three")
        assert all(wc.n_distinct(r) <= wc.SMALL_MAX_D and min(map(len, wc.sequences(r))) >= k for r in case["recs"])
        assert any(int(r[2].sum()) < len(case["names"]) for r in case["recs"])          # absent strains: consider_missing matters
        assert wc.predict_dedup(case["recs"]) == (16, 2)
        assert [m for _, m, _ in wc.runs(case)] == list(wc.MASKS) * 2


def test_pool_case_overflows_the_lds_pool():
    twelve, two = wc.pool_case()["recs"]
    words = [(len(s) + 31) // 32 for s in dict.fromkeys(wc.sequences(twelve))]
    assert len(words) == 12 and sum(sorted(words)[:6]) > wc.POOL_WORDS_SMALL          # eight groups (mask 0x7) do not fit
    assert all((len(s) + 31) // 32 > wc.POOL_WORDS_SMALL for s in wc.sequences(two)) and wc.n_distinct(two) == 2
    assert wc.eligible(two)
    case = wc.pool_case()
    assert int(two[2].sum()) < len(case["names"])                                      # absent strains: consider_missing on and off
    assert sorted({cm for _, _, cm in wc.runs(case)}) == [False, True]


def test_wide_case_holds_every_family():
    case = wc.wide_case()
    k = case["k"]
    recs = _by_name(case)
    assert all(65 <= wc.n_distinct(r) <= 200 for r in case["recs"]) and 200 <= len(case["names"]) <= 260
    assert all(wc.unit_contents_differ(r, k) for r in case["recs"])
    lens = {len(s) for s in wc.sequences(recs["trunc"])}
    assert len(lens) >= 40                                                              # nb differs, leading words equal
    t = set(wc.sequences(recs["tails"]))
    assert sum(1 for s in t if s + b"A" in t and s + b"AAAA" in t) >= 2                 # boundary and halo families
    assert any((len(s) - k + 1) % 64 == 0 and s + b"A" in t for s in t)                 # a tail that starts a unit of its own
    seqs = set(wc.sequences(recs["tandem"]))
    assert any(set(s) == {65} for s in seqs) and any(s[:2] == b"AT" and s == b"AT" * (len(s) // 2) for s in seqs)
    assert any(s[:64] == s[64:128] == s[128:192] and len(set(s)) == 4 for s in seqs)    # a 64-base period
    L = max(map(len, wc.sequences(recs["batches"])))
    Dp = (wc.n_distinct(recs["batches"]) + 31) // 32 * 32
    assert (L - k + 64) // 64 > wc.UNIT_PAIRS // Dp                                     # several batches of the class table
    masks = [(s, m) for s, m, cm in wc.runs(case) if not cm]
    # the unit-hash model: with the hash whole no cluster falls back, at mask 0 every one, and under nb_pair_mask the tails alone
    assert not any(wc.unit_fallback(r, k, wc.CONTROL) for r in case["recs"])
    assert all(wc.unit_fallback(r, k, 0) for r in case["recs"])
    assert [wc.unit_fallback(r, k, wc.nb_pair_mask(case)) for r in case["recs"]] == [r[1] == "tails" for r in case["recs"]]
    assert (wc.SITE_UNIT, wc.nb_pair_mask(case)) in masks
    # ... and under position_pair_mask the tandem cluster alone, and only because of the position: two units of equal bases
    pm = wc.position_pair_mask(case)
    assert [wc.unit_fallback(r, k, pm) for r in case["recs"]] == [r[1] == "tandem" for r in case["recs"]]
    assert not any(wc.unit_fallback(r, k, pm, position=False) for r in case["recs"])
    assert (wc.SITE_UNIT, pm) in masks
    assert (None, wc.WIDE_MASK) in masks and all((site, m) in masks for site in (wc.SITE_UNIT, wc.SITE_ROWS) for m in wc.MASKS[1:])


def test_rows_case_masks_and_keys():
    case = wc.rows_case()
    assert [(wc.n_distinct(r) + 31) // 32 for r in case["recs"]] == [3, 3, 4, 9]        # mask words: both step A widths
    census = [wc.mask_census(r, case["k"]) for r in case["recs"]]
    print(census)
    for (keys, masks), r in zip(census, case["recs"]):
        assert keys < wc.KEY_LIMIT                                                      # one work item
        assert masks >= wc.n_distinct(r)                                                # tree-like: multi-bit masks
    assert all(m < wc.MASK_TABLE_CAP // 2 for _, m in census[:3])                       # few masks: hits behind a collision
    assert census[3][1] > wc.MASK_TABLE_CAP                                             # a second round


def test_plot_table():
    text, strains, cols = wc.plot_table()
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    assert {r[0] for r in rows} == {"g0"} and {r[2] for r in rows} == {"1e-3"}
    assert {r[3] for r in rows} - set(strains) == {f"s{i}" for i in range(40, 45)}
    assert {r[0] for r in (ln.split("\t") for ln in wc.plot_table(True)[0].splitlines()[1:])} == {"g0", "g1"}
    assert np.all(np.array(cols) == [0, 3, 4, 1, 5, 2])
