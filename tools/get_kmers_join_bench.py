#!/usr/bin/env python3
"""panfeed-get-kmers end to end over a second-pass-shaped kmers.tsv: the device join against the pandas join.

Files (made once in --files-dir, by the package's own run_files): a pangenome of --clusters clusters x --samples strains,
every strain a target, so every row of kmers.tsv is a row of a selected cluster; kmers_to_hashes.tsv; an associations
file that lists every pattern of hashes_to_patterns.tsv, one in --pass-every of them under the threshold; and the same
tables device-gzipped (run_files(device_gzip=True)).
Per file (plain, device-gzipped) and route (the device join; --host-join, the pandas statements): get_kmers to a file,
wall time, median of --runs runs after a warm-up, with the range; the output's size and CRC32, which must not differ
between the routes; the device route's survey / join / inflate kernel times by HIP events and its bytes in.
--parent-root DIR measures the package of another checkout (the parent commit's, built) on the same files as well: its
one route.  The files' sizes and CRC32s are recorded by both, to show they are the same files.  Making the files, the
measurement and the parent's measurement are three child processes, each under a time limit of its own; one that fails
ends the run.

Writes bench.json and, with --parent-root, parent.json into --out-dir (default profiles/get_kmers_join/).  Usage:
    python tools/get_kmers_join_bench.py --files-dir DIR [--clusters 4] [--samples 250] [--runs 5] [--pass-every 25]
                                         [--parent-root DIR] [--out-dir DIR]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """the two sets of tables and the associations; nothing is made again when the directory has them"""
    d = args.files_dir
    done = os.path.join(d, "done")
    if os.path.exists(done):
        return
    from panfeed_amd import synth
    from panfeed_amd.pipeline import run_files
    os.makedirs(d, exist_ok=True)
    k, up, down = 31, 100, 100
    cl = synth.generate(args.clusters, args.samples, flank=up)
    csvp, _gffs, _fas = synth.write_pangenome(d, cl, missing_gene_rate=0.0)
    targets = tuple(cl[0].names)
    for label, kw in (("plain", {}), ("gz", {"device_gzip": True})):
        run_files(csvp, os.path.join(d, "gffs"), os.path.join(d, "out_" + label), klength=k, upstream=up, downstream=down,
                  targets=targets, batch_clusters=64, **kw)
    with open(os.path.join(d, "out_plain", "hashes_to_patterns.tsv")) as fh, open(os.path.join(d, "assoc.tsv"), "w") as out:
        fh.readline()
        out.write("variant\taf\tlrt-pvalue\tbeta\n")
        for i, line in enumerate(fh):
            out.write(f"{line.split(chr(9), 1)[0]}\t0.{i % 89 + 10}\t{'1e-5' if i % args.pass_every == 0 else '0.5'}\t{(i % 13) / 8}\n")
    open(done, "w").close()


def timed(args, kmers, kh, extra, label):
    from panfeed_amd import downstream
    out_path = os.path.join(args.files_dir, "annotated.tsv")
    argv = ["-a", os.path.join(args.files_dir, "assoc.tsv"), "-p", kh, "-k", kmers, "-t", "0.01"] + extra
    times, stats = [], None
    for i in range(args.runs + 1):
        t0 = time.perf_counter()
        with open(out_path, "w", encoding="utf-8") as out:
            rc = downstream.get_kmers(argv, out=out)
        dt = time.perf_counter() - t0
        assert rc == 0
        if i:
            times.append(dt)
        print(f"{label}: run {i}: {dt:.3f} s", flush=True)
    kj = getattr(downstream, "KmerJoin", None)
    if kj is not None and "--host-join" not in extra:
        stats = dict(kj.last_stats, device_bunches=kj.device_bunches, host_bunches=kj.host_bunches, host_runs=kj.host_runs)
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times,
            "output": file_id(out_path), "stats": stats}


STEP_LIMIT_S = {"files": 600, "measure": 900, "parent": 900}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files-dir", required=True)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pass-every", type=int, default=25)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built: its package is measured on the same files")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "get_kmers_join"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="(internal) the one step this process runs")
    args = ap.parse_args()
    if args.step is None:
        # every step that uses the GPU is a process of its own under its own time limit; a step that fails ends the run
        import subprocess
        for step in ("files", "measure") + (("parent",) if args.parent_root else ()):
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--step", step], timeout=STEP_LIMIT_S[step])
            if p.returncode != 0:
                sys.exit(f"step {step} ended with {p.returncode}: nothing more is run")
        return
    args.parent = args.step == "parent"
    root = os.path.abspath(args.parent_root if args.parent else REPO)
    sys.path.insert(0, root)
    import panfeed_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == root
    if args.step == "files":
        make_files(args)
        return
    out = os.path.join(args.out_dir, "parent.json" if args.parent else "bench.json")
    res = {"clusters": args.clusters, "samples": args.samples, "runs": args.runs, "parent": bool(args.parent), "files": []}
    for label, sub, ext in (("plain", "out_plain", ""), ("device-gzipped", "out_gz", ".gz")):
        kmers = os.path.join(args.files_dir, sub, "kmers.tsv" + ext)
        kh = os.path.join(args.files_dir, sub, "kmers_to_hashes.tsv" + ext)
        with (gzip.open if ext else open)(kmers, "rb") as fh:
            rows = sum(1 for _ in fh) - 1
        r = {"file": label, "kmers": file_id(kmers), "kmers_to_hashes": file_id(kh), "rows": rows}
        if args.parent:
            r["get_kmers"] = timed(args, kmers, kh, [], f"parent, {label}")
        else:
            r["device_join"] = timed(args, kmers, kh, [], f"device join, {label}")
            r["host_join"] = timed(args, kmers, kh, ["--host-join"], f"host join, {label}")
            assert r["device_join"]["output"] == r["host_join"]["output"], "the two routes' outputs differ"
        res["files"].append(r)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
