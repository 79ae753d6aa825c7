"""The hash-then-verify branches of the kernels, run with different content under one hash.

Five places are exact only because a content hash is followed by a compare of the content: the dedup pass's group table
(cluster_dedup_kernel, both size classes), the unit-class table (unit_class_kernel), the mask table of rows_kernel's mode 2,
the row filter's candidates (pf_rowfilter_scan and pf_rowfilter_scan_members) and the plot grid's name tables (pg_scan_kernel / pg_check_kernel).  With
64-bit hashes no input reaches those compares with two contents under one hash.  libpanfeed_hip_weakhash.so (built by
build() beside the shipped library, -DPF_WEAK_HASH) ANDs exactly those hashes with a mask; tests/weakhash_worker.py runs
it ONCE, in a process of its own, over tests/weak_hash_cases.py, and this module asserts run by run:

* the three texts equal the CPU oracle's byte for byte (by digest), at every mask, consider_missing on and off;
* at the control mask ~0 no compare fails and n_dedup_clusters / n_wide_clusters equal the shipped library's;
* at mask 0 the clusters that fall back are exactly those the case file predicts; at 0x7 some but not all;
* the unit-class and mask-table compares fail (their counters) when their hash alone is masked -- the dedup hash is left
  whole there, because a cluster whose dedup pass met a collision never reaches them;
* the row filter and the plot grid return what the shipped library returns, and two cluster names under one hash stop the
  scan with PF_ERR_CAPACITY.

If the worker exits abnormally every test here fails from that one run; nothing is started again."""
import json
import os
import subprocess
import sys

import pytest

import weak_hash_cases as wc
import weakhash_worker as ww
from conftest import REPO
from test_gpu_parity import _oracle_texts

pytestmark = pytest.mark.gpu

WORKER_TIMEOUT_S = 600
CASES = {c["name"]: c for c in wc.cases()}
RUNS = [(name, run) for name, c in CASES.items() for run in wc.runs(c)]


@pytest.fixture(scope="module")
def worker(tmp_path_factory):
    """the variant's results: one fresh child with its own time limit, never restarted"""
    out = tmp_path_factory.mktemp("weakhash")
    state = {"dir": str(out), "results": None, "error": None}
    try:
        p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "weakhash_worker.py"), str(out)], capture_output=True,
                           text=True, timeout=WORKER_TIMEOUT_S)
        if p.returncode != 0:
            state["error"] = f"weakhash_worker.py exited with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
        else:
            with open(os.path.join(str(out), "results.json")) as fh:
                state["results"] = json.load(fh)
            print(p.stdout.strip(), state["results"]["seconds"])
    except subprocess.TimeoutExpired as e:
        state["error"] = f"weakhash_worker.py did not finish in {WORKER_TIMEOUT_S} s:\n{(e.stderr or b'')[-4000:]}"
    return state


def _results(worker):
    if worker["error"]:
        pytest.fail(worker["error"], pytrace=False)
    return worker["results"]


_reference = {}


def reference(name, cm):
    """(oracle digests, Timing of the shipped library, digests of the shipped library with the unit view off) of a case,
    computed once"""
    if (name, cm) not in _reference:
        case = CASES[name]
        (ek, ekh, ehp), _ = _oracle_texts(case["recs"], stroi=set(case["stroi"]), klength=case["k"], canon=True,
                                          consider_missing=cm)
        oracle = {"kmers_tsv": ww.digest(ek), "kmers_to_hashes": ww.digest(ekh), "hashes_to_patterns": ww.digest(ehp)}
        shipped, timing = ww.engine_run(case, cm)
        assert shipped == oracle, f"{name}: the shipped library differs from the oracle"
        plain, _ = ww.engine_run(case, cm, unit_dedup=False)
        _reference[(name, cm)] = (oracle, timing, plain)
    return _reference[(name, cm)]


def test_worker_loaded_the_variant(worker):
    res = _results(worker)
    assert ww.VERSION_WORD in res["version"]
    assert len(res["runs"]) == len(RUNS)
    print("weak-hash worker, seconds per case:", res["seconds"])


def test_shipped_library_has_no_weak_hash_exports():
    from panfeed_amd import _lib
    assert os.path.basename(_lib.LIB_PATH) == "libpanfeed_hip.so"
    L = _lib.load()
    for name in ("pf_debug_set_hash_mask", "pf_debug_set_hash_mask_site", "pf_debug_weakhash_counts"):
        assert name not in _lib.EXPORTS
        with pytest.raises(AttributeError):
            getattr(L, name)
    assert ww.VERSION_WORD not in L.pf_version().decode()
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), ww.VARIANT))


@pytest.mark.parametrize("name,run", RUNS, ids=[wc.run_id(CASES[n], r) for n, r in RUNS])
def test_texts_are_the_oracles_whatever_the_hash(worker, name, run):
    res = _results(worker)
    case = CASES[name]
    sites, mask, cm = run
    got = res["runs"][wc.run_id(case, run)]
    oracle, shipped_timing, plain = reference(name, cm)
    cnt, tm = got["counters"], got["timing"]
    print(wc.run_id(case, run), cnt, tm)
    assert got["texts"]["hashes_to_patterns"] == oracle["hashes_to_patterns"]
    assert got["texts"]["kmers_to_hashes"] == oracle["kmers_to_hashes"]
    assert got["texts"]["kmers_tsv"] == oracle["kmers_tsv"]
    assert cnt["rowfilter"] == 0 and cnt["strain"] == 0
    # (rows_kernel's walk of a round's mask table never has to give up -- AT_SLOTS probes, 4 096 looks at a busy entry: the
    # table holds fewer entries than it has slots -- not even when every mask shares one hash)
    assert cnt["rows_gave_up"] == 0
    n_multi, n_single = wc.predict_dedup(case["recs"])
    if mask == wc.CONTROL:
        assert all(cnt[c] == 0 for c in wc.VERIFY_COUNTERS)
        assert tm["n_dedup_clusters"] == shipped_timing["n_dedup_clusters"]
        assert tm["n_wide_clusters"] == shipped_timing["n_wide_clusters"]
    if sites is None and mask != wc.CONTROL:
        # (a cluster whose dedup compare failed never reaches the unit-class or the mask table)
        assert mask == wc.WIDE_MASK or (cnt["unit"] == 0 and cnt["rows"] == 0)
    if sites is None and mask == 0:
        # one group per cluster: every cluster of two or more distinct (content, length) pairs falls back in the small class
        assert cnt["dedup_small"] == n_multi
        assert cnt["dedup_wide"] == 0
        assert tm["n_dedup_clusters"] == n_single
    if sites is None and mask != wc.CONTROL and name.startswith("small"):
        # whatever the mask, a cluster takes the view of distinct sequences unless a compare of its own failed: the clusters of
        # identical copies (no compare can fail) always do
        n_eligible = sum(wc.eligible(r) for r in case["recs"])
        assert tm["n_dedup_clusters"] == n_eligible - cnt["dedup_small"] and cnt["dedup_small"] <= n_multi
    if sites is None and mask == 0x7 and name.startswith("small"):
        assert 0 < cnt["dedup_small"] < n_multi
    if sites is None and mask in (0x7, wc.HIGH4) and not name.startswith("small"):
        assert cnt["dedup_small"] > 0
    if sites is None and mask == wc.WIDE_MASK:
        assert cnt["dedup_wide"] > 0
    if sites == wc.SITE_UNIT:
        assert cnt["dedup_small"] == 0 and cnt["dedup_wide"] == 0 and cnt["rows"] == 0
        assert tm["n_dedup_clusters"] == shipped_timing["n_dedup_clusters"]
        differ = sum(wc.unit_contents_differ(r, case["k"]) for r in case["recs"])
        if mask == 0:
            # one class per batch of unit positions: every cluster with two unit contents keeps its plain view, which is what
            # the shipped library computes with the unit view off
            assert cnt["unit"] == differ
            assert got["texts"] == plain
        # whatever the mask: the clusters in which two units of one table batch share the masked hash and differ
        assert cnt["unit"] == sum(wc.unit_fallback(r, case["k"], mask) for r in case["recs"])
        if mask in (0x7, wc.HIGH4):
            assert cnt["unit"] > 0
        if name.startswith("wide") and mask == wc.position_pair_mask(case):
            # only units 0 and 1 of the 64-base-period repeat meet, with equal bases: the position compare alone decides
            assert cnt["unit"] == 1 and not any(wc.unit_fallback(r, case["k"], mask, position=False) for r in case["recs"])
        if name.startswith("wide") and mask == wc.nb_pair_mask(case):
            # only X and X + 'AAAA' meet, with equal words: the nb compare alone sends the cluster back
            assert cnt["unit"] == 1 and [wc.unit_fallback(r, case["k"], mask) for r in case["recs"]] == [r[1] == "tails" for r in case["recs"]]
    if sites == wc.SITE_ROWS:
        assert cnt["dedup_small"] == 0 and cnt["dedup_wide"] == 0 and cnt["unit"] == 0
        assert tm["n_dedup_clusters"] == shipped_timing["n_dedup_clusters"]
        if mask in (0, 0x7):
            assert cnt["rows"] > 0
    if name.startswith("rows") and (sites == wc.SITE_ROWS or mask == wc.CONTROL):
        # tree260 carries more masks than a round's table takes: slots are handed to a second round (ENT_DEAD, table full)
        assert cnt["rows_handed_over"] > 0


# ------------------------------------------------------------------------------------------------- N4, N5
def _sorted_digest(text):
    return ww.digest("\n".join(sorted(text.splitlines())))


N4 = ww.n4_fixtures()


@pytest.mark.parametrize("fixture", range(len(N4)), ids=[f["case"] for f in N4])
@pytest.mark.parametrize("mask", ww.ROWFILTER_MASKS, ids=[f"{m:#x}" for m in ww.ROWFILTER_MASKS])
def test_rowfilter_candidates_are_verified(worker, tmp_path, mask, fixture):
    """every line of the golden files is a candidate under a masked key hash: the host's check of the key bytes keeps the
    lines the shipped library keeps (and the reference's tools print)"""
    res = _results(worker)
    got = res["rowfilter"][f"{fixture}-{mask:#x}"]
    paths, runs = ww.n4_files(str(tmp_path), N4[fixture])
    for run, g in zip(runs, got["runs"]):
        shipped = ww.n4_run(paths, run)
        assert g == shipped, (run["tool"], run["args"])
        assert g["lines"] == _sorted_digest(run["stdout"]) and g["rc"] == run["rc"]
    print("rowfilter", hex(mask), got["counters"])
    assert got["counters"]["rowfilter"] > 0
    assert got["counters"]["strain"] == 0


@pytest.mark.parametrize("mask", ww.ROWFILTER_MASKS, ids=[f"{m:#x}" for m in ww.ROWFILTER_MASKS])
def test_rowfilter_routes_verify_their_candidates_alike(worker, tmp_path, mask):
    """kmers_to_hashes.tsv of the first fixture as a plain file (pf_rowfilter_scan) and device-gzipped
    (pf_rowfilter_scan_members) under a masked key hash: both routes keep the rows the shipped library keeps of the plain
    file, and both reject the same number of candidates -- the plain route never scans the header line, the member route
    passes over the header's candidates before it counts"""
    res = _results(worker)
    got = res["rowfilter_routes"][f"{mask:#x}"]
    paths, _ = ww.n4_files(str(tmp_path), N4[0])
    plain = paths["kmers_to_hashes.tsv"]
    shipped = ww.route_rows(plain, ww.route_keys(plain))
    print("rowfilter routes", hex(mask), got)
    n_data = sum(1 for _ in open(plain, "rb")) - 1
    assert 0 < shipped["n_rows"] < n_data
    for route in ("plain", "members"):
        assert {k: got[route][k] for k in shipped} == shipped, route
    if mask == 0:
        # every data line is a candidate; those whose key is none of the keys are rejected by the bytes
        assert got["plain"]["rejects"] == n_data - shipped["n_rows"] > 0
    assert got["plain"]["rejects"] == got["members"]["rejects"]


@pytest.mark.parametrize("mask", ww.ROWFILTER_MASKS, ids=[f"{m:#x}" for m in ww.ROWFILTER_MASKS])
def test_plot_grid_strains_are_verified_by_bytes(worker, tmp_path, mask):
    """one cluster name, one p-value text, strains in the file that are not phenotype strains and share their hash with
    ones that are: the grids are the shipped library's"""
    res = _results(worker)
    got = res["plot"][f"one-{mask:#x}"]
    shipped = ww.plot_run(str(tmp_path), False)
    assert shipped["status"] == 0 and shipped["clusters"] == ["g0"] and shipped["pvalues"] == ["1e-3"]
    assert got["result"] == shipped
    print("plot grid", hex(mask), got["counters"])
    assert got["counters"]["strain"] > 0


def test_plot_grid_two_names_under_one_hash_stop_the_scan(worker, tmp_path):
    from panfeed_amd import _lib
    res = _results(worker)
    got = res["plot"]["two-0x0"]["result"]
    assert got["status"] == _lib.ERR_CAPACITY
    assert "share a 64-bit hash" in got["message"]
    assert got["grids"] is None
    shipped = ww.plot_run(str(tmp_path), True)                   # the same table is fine with the hash whole
    assert shipped["status"] == 0 and sorted(shipped["clusters"]) == ["g0", "g1"]
