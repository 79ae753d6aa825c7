#!/usr/bin/env python3
"""kmers.tsv rows of passing patterns only (Engine(passing_hashes=)): what the filter costs and what it saves.

The workload of tools/targets_stream_scale.py's comparison: M clusters x S strains (default 64 x 5 000, k = 21; 27 GB of
kmers.tsv), every strain a target strain, one batch through `Engine.run_batches(..., device_text=True, targets_sink=...)`
with a sink that only counts the bytes.  Legs, each a warm-up and then --runs runs (median and range):
  off     no filter
  every   every digest of the pattern table passes (the probe's cost per row: every listed row is still written)
  1pct    every hundredth digest
  empty   the empty list: no row passes
Per leg: seconds of the text stage and of the stream inside it, rows considered and kept, bytes out, and the mark and
index kernel's own milliseconds (pf_passing_mark_ms).

--files DIR adds one `pipeline.run_files` to real files under DIR (removed afterwards) on a pangenome of --files-clusters
x --files-samples written there, every strain a target: plain and `device_gzip`, unfiltered and -- not with --parent --
filtered by every hundredth hash of the unfiltered run's kmers_to_hashes.tsv.  One run each, wall seconds and bytes.

--parent measures the package of another checkout (--package-root, the parent commit's): the `off` leg only, which is
all that package has.

Prints one JSON line (and writes it to --out).  Usage:
    python tools/passing_rows_bench.py [--clusters 64] [--samples 5000] [--k 21] [--runs 5]
                                       [--parent --package-root DIR] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch(clusters, samples, k, flank, first):
    from panfeed_amd import synth
    from panfeed_amd.packing import build_batch_native
    t0 = time.time()
    cl = synth.generate(clusters, samples, first=first, flank=flank, n_rate=0.0)
    recs = [c.record() for c in cl]
    stroi = set(cl[0].names)
    hb = build_batch_native(recs, k, True, (samples + 31) // 32, stroi=stroi, first_ordinal=0)
    return hb, stroi, time.time() - t0


def one_run(eng, hb, filtered):
    n = [0]

    def sink(blk):
        n[0] += len(blk)
    t0 = time.perf_counter()
    outs = list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=sink))
    wall = time.perf_counter() - t0
    st = outs[0].stats
    res = {"wall_s": wall, "submit_s": eng.stages["submit_s"], "text_stage_s": eng.stages["text_s"],
           "stream_s": eng.render_targets_timing["render_s"], "bytes": n[0], "ranges": st["kmers_tsv_ranges"]}
    if filtered:
        ms = C.c_float()
        eng.L.pf_passing_mark_ms(eng.ctx, C.byref(ms))
        ps = eng.passing_stats()
        res.update(rows_considered=st["kmers_rows_considered"], rows_kept=st["kmers_rows_kept"], mark_index_ms=ms.value,
                   marked_kmers=ps[1], filter_device_bytes=ps[5])
    return res


def leg(make_engine, hb, passing, runs):
    eng = make_engine(passing)
    try:
        one_run(eng, hb, passing is not None)                    # warm-up
        got = [one_run(eng, hb, passing is not None) for _ in range(runs)]
    finally:
        eng.close()
    out = dict(got[-1])
    for key in ("wall_s", "text_stage_s", "stream_s", "submit_s") + (("mark_index_ms",) if passing is not None else ()):
        vals = [g[key] for g in got]
        out[key] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    out["digests"] = None if passing is None else len(passing)
    return out


def files_leg(root, clusters, samples, k, parent):
    """run_files to real files: {run: seconds, bytes of kmers.tsv, of the three files}"""
    import shutil
    from panfeed_amd import synth
    from panfeed_amd.pipeline import run_files
    os.makedirs(root, exist_ok=True)
    cl = synth.generate(clusters, samples, first=5 * 10 ** 6, flank=100, n_rate=0.001)
    csvp, gffs, _fas = synth.write_pangenome(root, cl)
    targets = tuple(cl[0].names)
    out, res = os.path.join(root, "out"), {}

    def run(name, **kw):
        shutil.rmtree(out, ignore_errors=True)
        t0 = time.perf_counter()
        stats = run_files(csvp, os.path.join(root, "gffs"), out, klength=k, upstream=100, downstream=100, targets=targets, **kw)
        secs = time.perf_counter() - t0
        sfx = ".gz" if kw.get("device_gzip") else ""
        sizes = [os.path.getsize(os.path.join(out, f + sfx)) for f in ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")]
        res[name] = {"seconds": secs, "kmers_tsv_bytes": sizes[0], "three_files_bytes": sum(sizes),
                     "rows_considered": stats.get("kmers_rows_considered"), "rows_kept": stats.get("kmers_rows_kept")}
        print(json.dumps({name: res[name]}), flush=True)
    run("warm_up_plain")
    run("plain")
    hashes = {}
    with open(os.path.join(out, "kmers_to_hashes.tsv")) as fh:
        next(fh)
        for line in fh:
            hashes[line.rstrip("\n").rsplit("\t", 1)[1]] = None
    passing = list(hashes)[::100]
    run("device_gzip", device_gzip=True)
    if not parent:
        res["passing_hashes"] = len(passing)
        run("plain_1pct", passing_hashes=passing)
        run("device_gzip_1pct", device_gzip=True, passing_hashes=passing)
    shutil.rmtree(root, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--flank", type=int, default=100)
    ap.add_argument("--budget", type=int, default=8 << 30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", action="store_true", help="measure only what an earlier package has: the off leg")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose panfeed_amd package is measured")
    ap.add_argument("--files", metavar="DIR", default=None, help="also one run_files to real files under DIR")
    ap.add_argument("--files-clusters", type=int, default=100)
    ap.add_argument("--files-samples", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import panfeed_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == os.path.abspath(args.package_root)
    from panfeed_amd.engine import Engine
    hb, stroi, gen_s = batch(args.clusters, args.samples, args.k, args.flank, 10 ** 6)

    def make_engine(passing):
        more = {} if passing is None else {"passing_hashes": passing}
        return Engine(klength=args.k, max_strains=(args.samples + 31) // 32 * 32, stroi=stroi,
                      targets_text_budget=args.budget, **more)
    res = {"shape": {"clusters": args.clusters, "samples": args.samples, "k": args.k, "flank": args.flank,
                     "budget": args.budget, "runs": args.runs}, "parent": bool(args.parent),
           "generate_pack_s": gen_s, "instances": int(hb.n_instances), "legs": {}}
    res["legs"]["off"] = leg(make_engine, hb, None, args.runs)
    print(json.dumps({"off": res["legs"]["off"]}), flush=True)
    if not args.parent:
        eng = make_engine(None)
        try:
            eng.submit_host_batch(hb)
            digests = [bytes(d) for d in eng.export_patterns()[0]]
        finally:
            eng.close()
        for name, passing in (("every", digests), ("1pct", digests[::100]), ("empty", [])):
            res["legs"][name] = leg(make_engine, hb, passing, args.runs)
            print(json.dumps({name: res["legs"][name]}), flush=True)
    if args.files:
        res["files"] = dict(files_leg(args.files, args.files_clusters, args.files_samples, args.k, args.parent),
                            clusters=args.files_clusters, samples=args.files_samples)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
