"""The weak-hash variant of the library in a process of its own, started once by tests/test_gpu_weak_hash.py.

    python tests/weakhash_worker.py OUTDIR

Points panfeed_amd._lib.LIB_PATH at libpanfeed_hip_weakhash.so before anything loads the library, checks that
pf_version() names the variant, goes through every run of tests/weak_hash_cases.py (and the row filter and plot grid
runs below, the row filter's two routes -- plain text and device-gzipped members -- among them) and writes OUTDIR/results.json: per run the digests of the three texts, the Timing fields and the counters of
pf_debug_weakhash_counts.  Asserts nothing about the results: the test module does, run by run.
"""
import ctypes as C
import hashlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import weak_hash_cases as wc  # noqa: E402
from device_gz_files import write_device_gz  # noqa: E402

VARIANT = "libpanfeed_hip_weakhash.so"
VERSION_WORD = "weak-hash"
ROWFILTER_MASKS = (0, 0x7)


def digest(text):
    return hashlib.sha256(text.encode() if isinstance(text, str) else text).hexdigest()


def text_digests(out):
    return {"kmers_tsv": digest(out.kmers_tsv), "kmers_to_hashes": digest(out.kmers_to_hashes),
            "hashes_to_patterns": digest(out.hashes_to_patterns)}


def engine_run(case, cm, **kw):
    """one fresh engine over the case's records: (texts' digests, Timing fields)"""
    from panfeed_amd.engine import Engine
    eng = Engine(**wc.engine_options(case, cm), **kw)
    try:
        out = eng.run(case["recs"])
    finally:
        eng.close()
    timing = {f: out.timing[f] for f in ("n_dedup_clusters", "n_wide_clusters", "n_items", "n_retried", "n_binned_clusters")}
    return text_digests(out), timing


def n4_fixtures():
    import gzip

    from conftest import GOLDEN
    with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as fh:
        return json.loads(fh.read().decode())["fixtures"]


def n4_files(outdir, fx):
    """kmers.tsv, kmers_to_hashes.tsv and the associations of one N4 fixture; its runs that the reference's tools ended
    with status 0 (the others stop at their options, before any file is read)"""
    from conftest import all_cases
    exp = {c["name"]: c for c in all_cases()}[fx["case"]]["expect"]
    os.makedirs(outdir, exist_ok=True)
    paths = {}
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        paths[name] = os.path.join(outdir, name)
        with open(paths[name], "w") as fh:
            fh.write(exp[name])
    paths["assoc"] = os.path.join(outdir, "assoc.tsv")
    with open(paths["assoc"], "w") as fh:
        fh.write(fx["associations"])
    runs = [r for r in fx["runs"] if r["rc"] == 0]
    return paths, runs


def n4_run(paths, run):
    """stdout of one golden run of panfeed-get-clusters / panfeed-get-kmers (both go through pf_rowfilter_scan)"""
    from panfeed_amd import downstream
    out = io.StringIO()
    argv = ["-a", paths["assoc"], "-p", paths["kmers_to_hashes.tsv"]] + run["args"]
    if run["tool"] == "get_kmers":
        argv += ["-k", paths["kmers.tsv"]]
    rc = (downstream.get_clusters if run["tool"] == "get_clusters" else downstream.get_kmers)(argv, out=out)
    return {"rc": int(rc or 0), "lines": digest("\n".join(sorted(out.getvalue().splitlines())))}


def route_keys(path):
    """every third of the distinct hashed_patterns of a kmers_to_hashes.tsv: the keys of route_rows, which keep some rows
    and leave the others to be rejected when every row is a candidate"""
    with open(path, "rb") as fh:
        lines = fh.read().split(b"\n")[1:-1]
    return sorted({ln.split(b"\t")[-1] for ln in lines})[::3]


def route_rows(path, keys, device_gunzip=None):
    """(header, rows) of one fresh last-field filter over the file, as digests, and the number of rows"""
    from panfeed_amd.downstream import RowFilter
    f = RowFilter(keys, first_field=False)
    try:
        header, rows = f.filter_file(path, device_gunzip=device_gunzip)
    finally:
        f.close()
    return {"header": digest(header), "rows": digest(rows), "n_rows": rows.count(b"\n")}


def plot_run(outdir, two_clusters):
    """the grids of weak_hash_cases.plot_table, or the error the scan stops with"""
    import numpy as np

    from panfeed_amd import _lib
    from panfeed_amd.plot import GridBuilder, significance_of
    text, strains, columns = wc.plot_table(two_clusters)
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "two.tsv" if two_clusters else "one.tsv")
    with open(path, "w") as fh:
        fh.write(text)
    gb = GridBuilder(strains, columns)
    try:
        try:
            gb.scan_file(path, block_bytes=64 << 10)
        except _lib.PanfeedHipError as e:
            return {"status": e.status, "message": str(e), "grids": None}
        gb.finish()
        gb.set_significance(significance_of(gb.pvalue_texts))
        ids = list(range(len(gb.clusters)))
        h = hashlib.sha256()
        for i, (key, cnt) in zip(ids, gb.grids(ids)):
            h.update(np.ascontiguousarray(key).tobytes() + np.ascontiguousarray(cnt).tobytes() + str(int(gb.min[i])).encode())
        return {"status": 0, "message": "", "grids": h.hexdigest(), "clusters": gb.clusters,
                "pvalues": [t.decode() for t in gb.pvalue_texts], "records": gb.n_records}
    finally:
        gb.close()


def main():
    outdir = sys.argv[1]
    from panfeed_amd import _lib
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), VARIANT)
    L = _lib.load()
    version = L.pf_version().decode()
    assert VERSION_WORD in version, version
    L.pf_debug_set_hash_mask.argtypes = [C.c_uint64]
    L.pf_debug_set_hash_mask_site.argtypes = [C.c_int, C.c_uint64]
    L.pf_debug_weakhash_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]

    def set_mask(sites, mask):
        _lib.check(L.pf_debug_set_hash_mask(wc.CONTROL))
        if sites is None:
            _lib.check(L.pf_debug_set_hash_mask(mask))
        else:
            _lib.check(L.pf_debug_set_hash_mask_site(sites, mask))

    def counters():
        buf = (C.c_uint64 * 8)()
        _lib.check(L.pf_debug_weakhash_counts(buf, 1))
        return dict(zip(wc.COUNTERS, [int(x) for x in buf]))

    from panfeed_amd.engine import Engine  # noqa: F401  (HIP initialised by the first engine, after the path was set)
    results = {"version": version, "runs": {}, "rowfilter": {}, "rowfilter_routes": {}, "plot": {}, "seconds": {}}
    t_all = time.time()
    for case in wc.cases():
        t0 = time.time()
        for run in wc.runs(case):
            sites, mask, cm = run
            set_mask(sites, mask)
            counters()
            texts, timing = engine_run(case, cm)
            results["runs"][wc.run_id(case, run)] = {"texts": texts, "timing": timing, "counters": counters()}
        results["seconds"][case["name"]] = round(time.time() - t0, 2)
    t0 = time.time()
    for i, fx in enumerate(n4_fixtures()):
        paths, runs = n4_files(os.path.join(outdir, f"n4_{i}"), fx)
        for mask in ROWFILTER_MASKS:
            set_mask(None, mask)
            counters()
            got = [n4_run(paths, r) for r in runs]
            results["rowfilter"][f"{i}-{mask:#x}"] = {"runs": got, "counters": counters()}
    # the first fixture's kmers_to_hashes.tsv by the row filter's two routes: the plain file (pf_rowfilter_scan) and the same
    # text device-gzipped (pf_rowfilter_scan_members), the file written before any hash is masked
    set_mask(None, wc.CONTROL)
    plain = os.path.join(outdir, "n4_0", "kmers_to_hashes.tsv")
    with open(plain, "rb") as fh:
        text = fh.read()
    cut = text.index(b"\n") + 1
    eng = Engine(klength=21, max_strains=32)
    try:
        write_device_gz(eng, plain + ".gz", text[:cut], text[cut:])
    finally:
        eng.close()
    keys = route_keys(plain)
    for mask in ROWFILTER_MASKS:
        set_mask(None, mask)
        counters()
        got = {}
        for route, path, kw in (("plain", plain, {}), ("members", plain + ".gz", {"device_gunzip": True})):
            got[route] = route_rows(path, keys, **kw)
            got[route]["rejects"] = counters()["rowfilter"]
        results["rowfilter_routes"][f"{mask:#x}"] = got
    for mask in ROWFILTER_MASKS:
        set_mask(None, mask)
        counters()
        got = plot_run(os.path.join(outdir, "plot"), False)
        results["plot"][f"one-{mask:#x}"] = {"result": got, "counters": counters()}
    set_mask(None, 0)
    results["plot"]["two-0x0"] = {"result": plot_run(os.path.join(outdir, "plot"), True), "counters": counters()}
    results["seconds"]["rowfilter_and_plot"] = round(time.time() - t0, 2)
    results["seconds"]["all"] = round(time.time() - t_all, 2)
    tmp = os.path.join(outdir, "results.json.tmp")
    with open(tmp, "w") as fh:
        json.dump(results, fh)
    os.replace(tmp, os.path.join(outdir, "results.json"))
    print("weakhash worker: %d runs in %.1f s" % (len(results["runs"]), time.time() - t_all), flush=True)


if __name__ == "__main__":
    main()
