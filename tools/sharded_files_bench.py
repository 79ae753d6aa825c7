#!/usr/bin/env python3
"""What a rank of a sharded run costs on ONE GPU (world 1 through panfeed_amd.sharded): nothing here is a multi-GPU number.

Part 1, the tools/gzip_device_bench.py pangenome (clusters x samples, a few target strains) through `run_files_sharded`
at world 1: plain, compress=True and device_gzip=True, wall seconds of --runs runs after a warm-up, and the files' bytes.
Part 2, one BASELINE configs[4]-shaped second-pass batch (every strain a target) through `run_records_sharded` at world 1
with a kmers.tsv budget: the peak device text, the ranges, the process's ru_maxrss.
Part 3, all patterns of a synthetic run through `Engine.render_pattern_rows` and through `Engine.stream_pattern_rows`,
plain and as gzip members: wall seconds, and the device bytes of the text (derived: the whole text for the renderer's
largest call, two slices for the stream).

Every part runs in a fresh child process (its ru_maxrss is its own; this process never touches the GPU).  --parent
measures a checkout of an earlier commit with what that commit has (--package-root <checkout>, built): no device_gzip, no
budget, no stream -- the yardsticks.  Writes one JSON file.  Usage:
    python tools/sharded_files_bench.py [--runs 5] [--out profiles/sharded_stream/bench.json]
    python tools/sharded_files_bench.py --parent --package-root <checkout> --out profiles/sharded_stream/parent.json
"""
import argparse
import json
import os
import resource
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def part_files(args):
    import torch

    from panfeed_amd import sharded, synth
    k, up, down = 31, 100, 100
    cl = synth.generate(args.clusters, args.samples, flank=up)
    d = tempfile.mkdtemp()
    csvp, _gffs, _fas = synth.write_pangenome(d, cl, missing_gene_rate=0.0)
    targets = tuple(cl[0].names[:args.targets])
    modes = [("plain", {}), ("compress", {"compress": True})] + ([] if args.parent else [("device_gzip", {"device_gzip": True})])
    out = {"clusters": args.clusters, "samples": args.samples, "targets": args.targets, "world": 1}
    for label, kw in modes:
        times, size, st = [], 0, {}
        for i in range(args.runs + 1):
            od = os.path.join(tempfile.mkdtemp(), "panfeed")
            t0 = time.perf_counter()
            st = sharded.run_files_sharded(csvp, os.path.join(d, "gffs"), od, 0, 1, None, torch.device("cuda", 0), klength=k,
                                           upstream=up, downstream=down, targets=targets, batch_clusters=64, **kw)
            dt = time.perf_counter() - t0
            size = sum(os.path.getsize(os.path.join(od, f)) for f in os.listdir(od))
            shutil.rmtree(os.path.dirname(od))
            if i:
                times.append(dt)
        out[label] = {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times,
                      "file_bytes": size, "text_bytes": st["bytes"],
                      "kmers_tsv_ranges": st.get("kmers_tsv_ranges"), "kmers_tsv_streamed": st.get("kmers_tsv_streamed")}
        print(label, json.dumps(out[label]), flush=True)
    shutil.rmtree(d)
    return out


def part_memory(args):
    import torch

    from panfeed_amd import sharded, synth
    cl = synth.generate(args.stream_clusters, args.stream_samples, first=10 ** 6, flank=100, n_rate=0.0)
    recs = [c.record() for c in cl]
    names = cl[0].names
    del cl
    od = tempfile.mkdtemp()
    kw = {} if args.parent else {"targets_text_budget": args.budget}
    t0 = time.perf_counter()
    st = sharded.run_records_sharded(recs, od, names, 0, 1, None, torch.device("cuda", 0), klength=21, targets=tuple(names),
                                     batch_clusters=args.stream_clusters, **kw)
    dt = time.perf_counter() - t0
    size = os.path.getsize(os.path.join(od, "kmers.tsv"))
    shutil.rmtree(od)
    return {"clusters": args.stream_clusters, "samples": args.stream_samples, "wall_s": dt, "kmers_tsv_file_bytes": size,
            "targets_text_budget": kw.get("targets_text_budget"), "kmers_tsv_ranges": st.get("kmers_tsv_ranges"),
            "kmers_tsv_streamed": st.get("kmers_tsv_streamed"),
            "kmers_tsv_peak_device_bytes": st.get("kmers_tsv_peak_device_bytes"),
            "ru_maxrss_bytes": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024}


def part_rows(args):
    import numpy as np

    from panfeed_amd import _lib, synth
    from panfeed_amd.engine import Engine
    S = args.rows_samples
    eng = Engine(klength=31, max_strains=(S + 31) // 32 * 32)
    done = 0
    while done < args.rows_clusters:                       # (generated a piece at a time: the records are large)
        n = min(250, args.rows_clusters - done)
        recs = [c.record() for c in synth.generate(n, S, first=done, flank=0)]
        for _ in eng.run_stream(recs, batch_clusters=125, defer_patterns=True, device_text=True):
            pass
        done += n
    md5, fs = eng.export_patterns()
    ids = np.argsort(fs, kind="stable").astype(np.uint32)
    per_row = 24 + 2 * eng.max_strains + 1
    out = {"clusters": args.rows_clusters, "samples": S, "patterns": int(len(ids))}

    def timed(fn):
        times, n = [], 0
        for i in range(args.runs + 1):
            t0 = time.perf_counter()
            n = fn()
            if i:
                times.append(time.perf_counter() - t0)
        return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times}, n
    r, n = timed(lambda: sum(len(b) for b in eng.render_pattern_rows(ids)))
    out["render_pattern_rows"] = dict(r, text_bytes=n, device_text_bytes=min(n, (256 << 20) // per_row * per_row))
    if not args.parent:
        count = [0]

        def sink(b):
            count[0] += len(b)
        r, res = timed(lambda: eng.stream_pattern_rows(ids, sink))
        assert res[0] == n
        out["stream_plain"] = dict(r, text_bytes=res[0], slices=res[2], device_text_bytes=2 * min(n, 64 << 20))
        _lib.check(eng.L.pf_set_device_gzip(eng.ctx, 1, 0))
        eng.device_gzip = True
        r, res = timed(lambda: eng.stream_pattern_rows(ids, sink))
        assert res[0] == n
        chunk = int(eng.L.pf_gzip_device_chunk_bytes())
        out["stream_device_gzip"] = dict(r, text_bytes=res[0], member_bytes=res[1], slices=res[2],
                                         device_text_bytes=2 * min(n, 64 << 20),
                                         device_member_bound_bytes="two slices' members: at most a ninth more than their text "
                                                                   f"plus the member frames ({chunk}-byte chunks)")
    eng.close()
    return out


PARTS = {"files": part_files, "memory": part_memory, "rows": part_rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--stream-clusters", type=int, default=4)
    ap.add_argument("--stream-samples", type=int, default=5000)
    ap.add_argument("--budget", type=int, default=1 << 30, help="targets_text_budget of part 2")
    ap.add_argument("--rows-clusters", type=int, default=2000)
    ap.add_argument("--rows-samples", type=int, default=1000)
    ap.add_argument("--parent", action="store_true", help="measure only what an earlier commit has")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose panfeed_amd is measured")
    ap.add_argument("--parts", default="files,memory,rows")
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sharded_stream", "bench.json"))
    args = ap.parse_args()
    root = os.path.abspath(args.package_root)
    if args.part:                                           # a child: one part, its result on the last line
        sys.path.insert(0, root)
        print("RESULT " + json.dumps(PARTS[args.part](args)), flush=True)
        return
    res = {"package_root_is_this_checkout": root == HERE, "parent": args.parent, "world": 1,
           "note": "one MI355X, world 1: not a multi-GPU measurement"}
    for part in args.parts.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part] + sys.argv[1:] + ["--package-root", root], cwd=root,
                           stdout=subprocess.PIPE, text=True)
        lines = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        res[part] = json.loads(lines[-1][7:]) if p.returncode == 0 and lines else {"failed": p.returncode,
                                                                                  "stdout_tail": p.stdout[-2000:]}
        print(part, json.dumps(res[part]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
