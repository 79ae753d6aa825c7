"""The size-class cases of tests/size_classes.py, held to their own claims and to the oracle without a GPU: the
mirrored constants equal the source, every case stands exactly on the quantity it claims and takes the route it names
by the model, the list covers every class and both sides of every term of the predicate, and the model's k-mers, rows
and kmers.tsv lines equal the oracle's texts on every case."""
import pytest

import kmer_content as kc
import size_classes as sc

CASES = sc.cases()


def _oracle(**kw):
    from oracle import oracle as po
    return po.OracleRun(**kw)


def test_mirrored_constants_equal_the_source():
    src, gone = sc.source_constants()
    assert set(src) == set(sc.MIRROR)
    wrong = {k: (sc.MIRROR[k], src[k]) for k in sc.MIRROR if sc.MIRROR[k] != src[k]}
    assert not wrong, f"mirrored constants differ from the source (mirror, source): {wrong}"
    assert not gone, "expressions the model restates are no longer in the source:\n" + "\n".join(gone)


def test_derived_sizes():
    """what the cases' numbers rest on: the table sizes per key width, their limits, which small tables exist, and the
    relations between the limits that the kernels' own comments state"""
    F = sc.MIRROR
    assert [sc.nslots_max(kw) for kw in (1, 2, 3, 4)] == [9600, 6400, 4800, 3840]
    assert [sc.insert_limit(n) for n in (4096, 6144, 9600, 6400, 4800, 3840)] == [1920, 3968, 7424, 4224, 2624, 1664]
    assert [kc.key_words(k) for k in (31, 63, 94, 126)] == [1, 2, 3, 4]
    assert sc.nslots_max(1) <= F["SLOT_AT"] and F["SORT_MAX"] >= sc.insert_limit(sc.nslots_max(1))
    assert F["FUSED_MAX_EXTRA"] == F["DEDUP_EX_LDS"]                  # one case pair stands on both
    assert F["FinHuge"]["DW"] * 32 < F["DENSE_WORDS"] * 32
    assert max(F[c]["MR"] for c in ("FinSmall", "FinLarge", "FinLargeM", "FinHuge")) < F["DEDUP_MROWS"]
    for cfg in ("FinSmall", "FinLarge", "FinLargeM", "FinHuge"):
        assert F[cfg]["ATL"] < F[cfg]["AT"] - 1                       # (the last position means "not in the table")
    assert F["AT_LIMIT"] < F["AT_SLOTS"] and F["LT_LIMIT"] < F["LT_SLOTS"]
    # a 4 096-slot table exists for one- and two-word keys, a 6 144-slot one for one-word keys only
    assert [[sc.nslots_max(kw) > t + F["INSERT_SLACK"] for t in F["SMALL_TABLES"]] for kw in (1, 2, 3, 4)] == \
        [[True, True], [True, False], [False, False], [False, False]]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_stands_on_its_claim(case):
    q = sc.quant(case)
    r = sc.expected_route(q, case.kind.k)
    name, value = case.claim
    assert getattr(q, name) == value, f"{case}: {name} is {getattr(q, name)}, the case claims {value}"
    assert (r.cls, r.mode) == case.route, f"{case}: the model routes it to {(r.cls, r.mode)}, the case names {case.route}"
    for field in ("nparts", "nslots"):
        if field in case.extra:
            assert getattr(r, field) == case.extra[field], (field, getattr(r, field))
    if "patterns" in case.extra:
        assert q.patterns == case.extra["patterns"] and q.patterns == q.masks
    assert q.W == case.kind.W and q.mult == (1 if case.kind.canon else 2)
    # only the cases that say so run a table past its limit; no several-partition case comes near it
    assert r.overflows == any(e.startswith("unique>limit(NS):past") for e in case.edges), (q.unique, r.nslots)
    if r.nparts > 1:
        assert q.unique / r.nparts < 0.8 * sc.insert_limit(r.nslots)
    assert r.planned == (r.cls in (sc.SMALL, sc.LARGE, sc.HUGE))
    assert r.binned == (r.nparts >= 3)
    if "nex_items:1" in case.edges or "nex<=FUSED_MAX_EXTRA:out" in case.edges:
        assert r.nex_items == 1
    if "nex_items:2" in case.edges:
        assert r.nex_items == 2


def test_seam_and_last_ordinal_cases():
    """FinHuge keeps 16-bit prefix counts per half of its bitmap: first occurrences on either side of dense ordinal
    65 536 from one substitution, none at all in the upper half, and the class's last ordinal occupied"""
    k, half = 31, sc.MIRROR["FinHuge"]["DW"] * 16
    first = set(sc.quant(sc.CASES["seam_straddled"]).first_ords)
    assert set(range(half - k // 2, half + k // 2 + 1)) <= first
    first = sc.quant(sc.CASES["seam_upper_half_empty"]).first_ords
    assert max(first) < half and len(first) > 2 * k
    q = sc.quant(sc.CASES["dense_huge_last"])
    assert max(q.first_ords) == q.dense - 1 == 2 * half - 3


def test_cases_cover_every_class_and_both_sides_of_every_term():
    claimed = [e for cs in CASES for e in cs.edges]
    assert sorted(set(claimed)) == sorted(set(sc.EDGES)), (set(sc.EDGES) - set(claimed), set(claimed) - set(sc.EDGES))
    routes = {cs.route for cs in CASES}
    assert routes == {(c, 1) for c in (sc.GENERAL, sc.SMALL, sc.LARGE, sc.LARGE_MULTI, sc.HUGE)} | {(sc.GENERAL, 2)}
    tables = {(kc.key_words(cs.kind.k), sc.expected_route(sc.quant(cs), cs.kind.k).nslots) for cs in CASES}
    assert tables >= {(1, 4096), (1, 6144), (1, 9600), (2, 4096), (2, 6400), (3, 4800), (4, 3840)}
    assert (2, 6144) not in tables
    assert {sc.expected_route(sc.quant(cs), cs.kind.k).nparts for cs in CASES} >= {1, 2, 3, 4}
    assert all(len(sc.cases(kind)) >= 1 for kind in sc.KINDS)
    assert len({cs.name for cs in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_texts_equal_the_oracle(case):
    """kmer_content's model of the reference (k-mers in dict order, each k-mer's sample set, every kmers.tsv line)
    against the oracle's three texts"""
    kd = case.kind
    rec = sc.build(case)
    run = _oracle(**kd.opts())
    run.feed([rec])
    kt, kh, hp = run.texts()
    models = kc.check_kmers(kh, hp, kt, [rec], kd.k, kd.canon, stroi=kd.opts()["stroi"])
    q = sc.quant(case)
    assert len(models[0].kmers) == q.unique + q.nex
    assert run.stats()["unique_kmers"] == q.unique + q.nex
