#!/usr/bin/env python3
"""The large-member gunzip route (--gpu-gunzip-large) against the host's gzip, on the files other writers make.

Text: the kmers.tsv of one second-pass batch (tools/gunzip_device_bench.py's: 4 clusters x 5 000 samples, every strain a
target: 2.36 GB).  Files of it:
  one_member   one whole-file gzip member with FLG = FNAME, as gzip.open(path, "wb") -- the reference's --compress -- writes
  host_members what this project's --compress writes: zlib members of 4 MiB of text (output.ParallelGzipWriter)
Per file, wall seconds of RowFilter.filter_file (a key no row has: the whole file is inflated and scanned) and of
KmerJoin.survey_file, a fresh owner each time, --runs runs after a warm-up, with the route's piece counters and the device
time of its four passes.  --parent measures the package of another checkout (--package-root, the parent commit's) on the
same files: filter_file(path) and survey_file(path), which go through the host's gzip there.  The files' sizes and CRC32s
are recorded by both.

The tool is a driver: each step -- make the files, measure -- runs in a child process of its own under a time limit, and a
step that fails or runs out of time ends the run.  Usage:
    python tools/gunzip_large_bench.py --dir DIR [--stream-clusters 4] [--stream-samples 5000] [--runs 5]
                                       [--parent --package-root DIR] [--out FILE] [--step-seconds 500]
"""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("one_member", "host_members")


def file_id(path):
    crc, n = 0, 0
    with open(path, "rb") as fh:
        while True:
            b = fh.read(1 << 24)
            if not b:
                break
            crc, n = zlib.crc32(b, crc), n + len(b)
    return {"bytes": n, "crc32": crc}


def paths(d):
    return {"plain": os.path.join(d, "kmers.tsv"), "one_member": os.path.join(d, "one_member", "kmers.tsv.gz"),
            "host_members": os.path.join(d, "host_members", "kmers.tsv.gz")}


def make(args):
    """the plain stream, then the two .gz files of it, written on the host"""
    sys.path.insert(0, REPO)
    from panfeed_amd.engine import Engine
    from panfeed_amd.output import KMERS_TSV_HEADER, ParallelGzipWriter
    from tools.targets_stream_scale import batch
    p = paths(args.dir)
    for f in FILES:
        os.makedirs(os.path.dirname(p[f]), exist_ok=True)
    hb, stroi, _gen = batch(args.stream_clusters, args.stream_samples, 21, 100, 10 ** 6)
    eng = Engine(klength=21, max_strains=(args.stream_samples + 31) // 32 * 32, stroi=stroi)
    try:
        with open(p["plain"], "wb") as w:
            w.write(KMERS_TSV_HEADER.encode())
            list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=lambda blk: w.write(bytes(blk))))
    finally:
        eng.close()
    t0 = time.perf_counter()
    with open(p["plain"], "rb") as src, gzip.open(p["one_member"], "wb", compresslevel=6) as one:
        pw = ParallelGzipWriter(p["host_members"])
        while True:
            b = src.read(16 << 20)
            if not b:
                break
            one.write(b)
            pw.write(b.decode())
        pw.close()
    print(json.dumps({"made": {k: file_id(v) for k, v in p.items()}, "compress_s": time.perf_counter() - t0}), flush=True)


def timed(run, runs):
    times, last = [], None
    for i in range(runs + 1):
        t0 = time.perf_counter()
        last = run()
        dt = time.perf_counter() - t0
        if i:
            times.append(dt)
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times, **last}


def measure(args):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(args.package_root))
    import panfeed_amd
    from panfeed_amd.downstream import KmerJoin, RowFilter
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == os.path.abspath(args.package_root)
    p = paths(args.dir)
    with open(p["plain"], "rb") as fh:
        cluster = fh.read(1 << 16).split(b"\n")[1].split(b"\t")[0]
    kw = {} if args.parent else {"large_members": True}
    res = {"parent": bool(args.parent), "runs": args.runs, "plain": file_id(p["plain"]), "files": []}

    def filter_file(path):
        f = RowFilter(["no_such_key"], first_field=True)
        try:
            got = f.filter_file(path, **kw)
            out = {"rows_bytes": len(got[1]), "stats": f.stats()}
            if not args.parent:
                out["large"] = f.large_stats()
            return out
        finally:
            f.close()

    def survey(path):
        kj = KmerJoin([(cluster, 0)], 1, [], [], [], b"")
        try:
            plan = kj.survey_file(path, **kw)
            out = {"rows": plan[0]["rows"], "stats": kj.stats()}
            if not args.parent:
                out["large"] = kj.large_stats()
            return out
        finally:
            kj.close()

    for name in FILES:
        one = {"file": name, "gz": file_id(p[name])}
        one["filter_file"] = timed(lambda: filter_file(p[name]), args.runs)
        one["survey_file"] = timed(lambda: survey(p[name]), args.runs)
        if not args.parent:
            for k in ("filter_file", "survey_file"):
                assert one[k]["stats"]["text_bytes_inflated"] == res["plain"]["bytes"], "the route did not take the whole file"
                lg = one[k]["large"]
                total = lg["find_ms"] + lg["marker_ms"] + lg["chain_ms"] + lg["bytes_ms"]
                one[k]["pass_share"] = {s: lg[s + "_ms"] / total for s in ("find", "marker", "chain", "bytes")}
        res["files"].append(one)
        print(json.dumps(one), flush=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", required=True, help="where the files are made and read")
    ap.add_argument("--stream-clusters", type=int, default=4)
    ap.add_argument("--stream-samples", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", action="store_true", help="measure filter_file(path) and survey_file(path): all an earlier package has")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose panfeed_amd package is measured")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-seconds", type=int, default=500, help="time limit of each step")
    ap.add_argument("--step", choices=("make", "measure"), default=None, help="(the driver's children)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(REPO, "profiles", "gunzip_large", "parent.json" if args.parent else "bench.json")
    if args.step:
        return (make if args.step == "make" else measure)(args)
    steps = ([] if os.path.exists(paths(args.dir)["host_members"]) else ["make"]) + ["measure"]
    for step in steps:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:], timeout=args.step_seconds)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: nothing more is run", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except subprocess.TimeoutExpired as e:
        print(f"a step ran past its {e.timeout} s: nothing more is run", file=sys.stderr)
        sys.exit(124)
