#!/usr/bin/env python3
"""The first step of both downstream tools, `_associations`, alone, over a pyseer-shaped associations table: the device
filter with pandas on the kept lines against pandas on the whole file.

Files (made once in --files-dir, from a seed): eight columns -- variant (a base64 hash of 24 characters), af,
filter-pvalue, lrt-pvalue, beta, beta-std-err, intercept, notes --, --rows rows, cells printed with %.2E.  `uniform.tsv`
has p-values uniform in (0, 1), `loguniform.tsv` log-uniform over 1e-12 .. 1.  Three regimes:
    a  uniform.tsv     -t 1e-5   about rows / 100 000 rows kept
    b  loguniform.tsv  -t 1e-8   a third kept
    c  uniform.tsv     -t 1      every row kept: pandas parses all of them either way
Per regime: `_associations(args)` to a -o file, wall time, one warm-up and --runs runs, their median and range; the kept
table's rows and the -o file's size and CRC32; the device pass's own time by HIP events and the bytes it scanned.  This
commit's package is also timed with --host-associations (the parent's statements in this commit), and the -o files of the
two routes must not differ.  --parent-root DIR measures the package of another checkout (the parent commit's, where
`_associations` is the pandas statements; it needs no build for that) on the same files in the same sitting.  Making the
files, the measurement and the parent's measurement are three child processes, each under a time limit of its own; one
that fails ends the run.

Writes bench.json and, with --parent-root, parent.json into --out-dir (default profiles/associations_filter/).  Usage:
    python tools/associations_bench.py --files-dir DIR [--rows 2000000] [--runs 3] [--parent-root DIR] [--out-dir DIR]
"""
import argparse
import base64
import hashlib
import json
import os
import random
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = (("a", "uniform.tsv", 1e-5), ("b", "loguniform.tsv", 1e-8), ("c", "uniform.tsv", 1.0))
HEADER = "variant\taf\tfilter-pvalue\tlrt-pvalue\tbeta\tbeta-std-err\tintercept\tnotes\n"
NOTES = ("", "", "", "bad-chisq", "high-bse")


def file_id(path):
    crc, n = 0, 0
    with open(path, "rb") as fh:
        while True:
            b = fh.read(1 << 24)
            if not b:
                break
            crc, n = zlib.crc32(b, crc), n + len(b)
    return {"bytes": n, "crc32": crc}


def make_files(args):
    """the two tables; nothing is made again when the directory has them"""
    d = args.files_dir
    done = os.path.join(d, f"done_{args.rows}")
    if os.path.exists(done):
        return
    os.makedirs(d, exist_ok=True)
    for name, seed in (("uniform.tsv", 11), ("loguniform.tsv", 12)):
        rnd = random.Random(seed)
        with open(os.path.join(d, name), "w") as out:
            out.write(HEADER)
            for i in range(args.rows):
                h = base64.b64encode(hashlib.md5(b"%d-%d" % (seed, i)).digest()).decode()
                p = rnd.random() if name == "uniform.tsv" else 10 ** rnd.uniform(-12, 0)
                out.write("%s\t%.2E\t%.2E\t%.2E\t%.2E\t%.2E\t%.2E\t%s\n" % (h, rnd.uniform(0.01, 0.5), min(1.0, p * 3), p, rnd.gauss(0, 1),
                                                                          rnd.uniform(0.05, 2), rnd.gauss(0, 1), NOTES[i % 5]))
    open(done, "w").close()


def timed(args, path, thr, host, label):
    from panfeed_amd import downstream
    out_path = os.path.join(args.files_dir, "filtered.tsv")
    ns = argparse.Namespace(associations=path, threshold=thr, column="lrt-pvalue", output=out_path, device=0, host_gunzip=False,
                            host_associations=host)
    times, rows = [], None
    af = getattr(downstream, "AssocFilter", None)
    before = af.device_files if af is not None else 0
    for i in range(args.runs + 1):
        t0 = time.perf_counter()
        a, passing = downstream._associations(ns)
        dt = time.perf_counter() - t0
        rows = len(a)
        if i:
            times.append(dt)
        print(f"{label}: run {i}: {dt:.3f} s, {rows} rows", flush=True)
    stats = dict(af.last_stats, device_runs=af.device_files - before) if af is not None and not host else None
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times, "rows_kept": rows,
            "passing": len(passing), "output": file_id(out_path), "stats": stats}


STEP_LIMIT_S = {"files": 600, "measure": 900, "parent": 600}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files-dir", required=True)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit: its package is measured on the same files")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "associations_filter"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="(internal) the one step this process runs")
    args = ap.parse_args()
    if args.step is None:
        # every step is a process of its own under its own time limit; a step that fails ends the run
        import subprocess
        for step in ("files", "measure") + (("parent",) if args.parent_root else ()):
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--step", step], timeout=STEP_LIMIT_S[step])
            if p.returncode != 0:
                sys.exit(f"step {step} ended with {p.returncode}: nothing more is run")
        return
    parent = args.step == "parent"
    root = os.path.abspath(args.parent_root if parent else REPO)
    sys.path.insert(0, root)
    import panfeed_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == root
    if args.step == "files":
        make_files(args)
        return
    import pandas
    out = os.path.join(args.out_dir, "parent.json" if parent else "bench.json")
    res = {"rows": args.rows, "runs": args.runs, "parent": parent, "pandas": pandas.__version__, "regimes": []}
    for regime, name, thr in REGIMES:
        path = os.path.join(args.files_dir, name)
        r = {"regime": regime, "file": name, "threshold": thr, "table": file_id(path)}
        if parent:
            r["associations"] = timed(args, path, thr, False, f"parent, {regime}")
        else:
            r["device_route"] = timed(args, path, thr, False, f"device route, {regime}")
            r["host_route"] = timed(args, path, thr, True, f"host route, {regime}")
            assert r["device_route"]["output"] == r["host_route"]["output"], "the two routes' -o files differ"
            assert r["device_route"]["stats"]["device_runs"] == args.runs + 1, "a run went through pandas whole"
        res["regimes"].append(r)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
