"""The post-scan size classes at each class's last and first size (tests/size_classes.py) on the GPU.  Every case runs
through Engine.run four ways -- as shipped, planned on the device, without the unit view, without the dedup pass -- each
on a fresh engine (a fresh context has learned no line for the key-partition estimate).  The three texts equal the
oracle's byte for byte in all four, pattern_model.check_rows passes on the GPU's own text, and in the first two the route
the library reports through pf_debug_cluster_routes equals the model's, cluster for cluster, and the two equal each
other: host planning and device planning are two copies of one rule.  Then all cases of a kind go through as one batch,
in order and reversed, so that the classes run side by side."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import pattern_model as pm
import size_classes as sc

gpu = pytest.mark.gpu

CASES = sc.cases()
MODES = [("shipped", {}), ("device_plan", dict(device_plan=True)), ("no_unit_view", dict(unit_dedup=False)),
         ("no_dedup", dict(dedup=False))]


def _engine(kd, **mode):
    from panfeed_amd.engine import Engine
    return Engine(max_strains=kd.max_strains, max_items=64, **kd.opts(), **mode)


@lru_cache(maxsize=None)
def _expect(names):
    """the oracle's texts of these cases as one run, and their unique k-mers"""
    from oracle import oracle as po
    kd = sc.CASES[names[0]].kind
    run = po.OracleRun(**kd.opts())
    run.feed([sc.build(sc.CASES[n]) for n in names])
    return run.texts(), run.stats()["unique_kmers"]


def _routes(eng, n):
    from panfeed_amd import _lib
    route = np.zeros(n, dtype=np.uint8)
    nparts, nslots, attempts = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    _lib.check(eng.L.pf_debug_cluster_routes(eng.ctx, n, *(a.ctypes.data_as(C.c_void_p) for a in (route, nparts, nslots, attempts))))
    return [dict(cls=int(r) & 7, mode=(int(r) >> 3) & 3, first=int(r) >> 5, nparts=int(p), nslots=int(s), attempts=int(a))
            for r, p, s, a in zip(route, nparts, nslots, attempts)]


def _run(kd, names, **mode):
    eng = _engine(kd, **mode)
    out = eng.run([sc.build(sc.CASES[n]) for n in names])
    routes = _routes(eng, len(names))
    eng.close()
    (ek, ekh, ehp), unique = _expect(tuple(names))
    what = f"{names[0] if len(names) == 1 else kd.name} {mode}"
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, kd.S, False)
    assert out.hashes_to_patterns == ehp, f"{what}: hashes_to_patterns.tsv"
    assert out.kmers_to_hashes == ekh, f"{what}: kmers_to_hashes.tsv"
    assert out.kmers_tsv == ek and len(ek) > 0, f"{what}: kmers.tsv"
    assert out.stats["unique_kmers"] == unique
    return out, routes


def _check_route(case, got, what, wrong):
    """a cluster's reported route against the model's; what differs is added to `wrong`"""
    r = sc.expected_route(sc.quant(case), case.kind.k)
    try:
        _assert_route(case, r, got, what)
    except AssertionError as e:
        wrong.append(str(e).splitlines()[0])
    return r


def _assert_route(case, r, got, what):
    assert got["mode"] == r.mode, f"{what}: view mode {got['mode']}, the model says {r.mode}"
    assert got["first"] == r.cls, f"{what}: the first attempt went to class {got['first']}, the model says {r.cls}"
    if r.overflows:
        assert got["attempts"] >= 2, f"{what}: {sc.quant(case).unique} keys past a limit of {sc.insert_limit(r.nslots)} in one attempt"
        assert got["nparts"] >= 2
    else:
        assert got["attempts"] == 1, f"{what}: {got['attempts']} attempts"
        assert (got["cls"], got["nparts"], got["nslots"]) == (r.cls, r.nparts, r.nslots), \
            f"{what}: (class, partitions, slots) {(got['cls'], got['nparts'], got['nslots'])}, the model says {(r.cls, r.nparts, r.nslots)}"


@gpu
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_four_ways(case):
    kd = case.kind
    seen, wrong = {}, []
    for tag, mode in MODES:
        out, routes = _run(kd, [case.name], **mode)
        seen[tag] = routes[0]
        t = out.timing
        if tag in ("shipped", "device_plan"):
            r = _check_route(case, routes[0], f"{case} {tag}", wrong)
            want = dict(n_device_planned=1 if tag == "device_plan" and r.planned else 0, n_dedup_clusters=1,
                        n_wide_clusters=1 if r.mode == 2 else 0)
            if not r.overflows:
                want.update(n_retried=0, n_items=r.nparts + r.nex_items, n_binned_clusters=1 if r.binned else 0)
            got = {f: t[f] for f in want}
            if got != want:
                wrong.append(f"{case} {tag}: timing counters {got}, the model says {want}")
        elif tag == "no_dedup":
            assert (routes[0]["cls"], routes[0]["mode"]) == (sc.GENERAL, 0) and t["n_dedup_clusters"] == 0
    if seen["shipped"] != seen["device_plan"]:
        wrong.append(f"host planning and device planning disagree: {seen['shipped']} and {seen['device_plan']}")
    assert not wrong, "\n".join(wrong)


@gpu
@pytest.mark.parametrize("order", ["in_order", "reversed"])
@pytest.mark.parametrize("kind", sorted(sc.KINDS))
def test_kind_as_one_batch(kind, order):
    """all cases of a kind in one submit: every class beside the others, planned by the host and by the device"""
    kd = sc.KINDS[kind]
    names = [cs.name for cs in sc.cases(kind)]
    if order == "reversed":
        names = names[::-1]
    seen, wrong = {}, []
    for tag, mode in MODES[:2]:
        out, routes = _run(kd, names, **mode)
        seen[tag] = routes
        planned = 0
        for n, got in zip(names, routes):
            planned += _check_route(sc.CASES[n], got, f"{n} in the batch of {kind}, {tag}", wrong).planned
        if out.timing["n_device_planned"] != (planned if tag == "device_plan" else 0):
            wrong.append(f"{kind} {tag}: {out.timing['n_device_planned']} clusters planned on the device, the model says {planned}")
    for n, a, b in zip(names, seen["shipped"], seen["device_plan"]):
        if a != b:
            wrong.append(f"{n}: host planning and device planning disagree: {a} and {b}")
    assert not wrong, "\n".join(wrong)


@gpu
def test_route_hook_refuses_what_it_cannot_answer():
    """no batch yet: PF_ERR_STATE; another cluster count than the last batch's: PF_ERR_ARG; arrays may be left out"""
    from panfeed_amd import _lib
    kd = sc.KINDS["k31"]
    eng = _engine(kd)
    with pytest.raises(_lib.PanfeedHipError) as e:
        _routes(eng, 1)
    assert e.value.status == _lib.ERR_STATE
    eng.run([sc.build(sc.CASES["upper_mask_word_present"])])
    with pytest.raises(_lib.PanfeedHipError) as e:
        _routes(eng, 2)
    assert e.value.status == _lib.ERR_ARG
    attempts = np.zeros(1, dtype=np.uint32)
    _lib.check(eng.L.pf_debug_cluster_routes(eng.ctx, 1, None, None, None, attempts.ctypes.data_as(C.c_void_p)))
    assert attempts[0] == 1 and _routes(eng, 1)[0]["cls"] == sc.SMALL
    eng.close()
