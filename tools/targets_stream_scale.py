#!/usr/bin/env python3
"""kmers.tsv of BASELINE configs[4]'s second pass at full size, streamed within a device-memory budget.

M clusters x S strains (default 256 x 5 000, k = 21), every strain a target strain: one batch through
`Engine.run_batches(..., device_text=True, targets_sink=...)` -- what `pipeline.run_files` (and so `python -m panfeed_amd
--targets ...`) does with it -- with a sink that only counts the bytes.  At the default budget (8 GiB) the text
(~150 GB) goes out in ranges (pf_kmers_tsv_stream_begin / _next); the single-buffer path (pf_render_kmers_tsv_device)
would need it in one device buffer.

--compare M2: also time the single-buffer path and the streamed path on an M2-cluster batch (one process, one context),
for the per-byte rate of both.

Prints one JSON line (and writes it to --out).  Usage:
    python tools/targets_stream_scale.py [--clusters 256] [--samples 5000] [--k 21] [--compare 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def batch(clusters, samples, k, flank, first):
    from panfeed_amd import synth
    from panfeed_amd.packing import build_batch_native
    t0 = time.time()
    cl = synth.generate(clusters, samples, first=first, flank=flank, n_rate=0.0)
    recs = [c.record() for c in cl]
    stroi = set(cl[0].names)
    W = (samples + 31) // 32
    hb = build_batch_native(recs, k, True, W, stroi=stroi, first_ordinal=0)
    return hb, stroi, time.time() - t0


def streamed(eng, hb, label):
    """one batch through run_batches with a counting sink: bytes, ranges, peak device text, seconds of the text stage"""
    n = [0]

    def sink(blk):
        n[0] += len(blk)
    outs = list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=sink))
    st, stages = outs[0].stats, eng.stages
    text_s = stages["text_s"]
    return {"path": label, "bytes": n[0], "ranges": st["kmers_tsv_ranges"],
            "peak_device_text_bytes": st["kmers_tsv_peak_device_bytes"], "submit_s": stages["submit_s"],
            "text_stage_s": text_s, "marshal_s": eng.render_targets_timing["marshal_s"],
            "stream_s": eng.render_targets_timing["render_s"],
            "GBps_text_out": n[0] / eng.render_targets_timing["render_s"] / 1e9}


def single_buffer(eng, hb):
    eng.submit_host_batch(hb)
    t0 = time.time()
    dt = eng.render_targets_device(hb)
    t1 = time.time()
    n = 0
    for blk in dt.chunks():
        n += len(blk)
    t2 = time.time()
    return {"path": "single_buffer", "bytes": n, "marshal_s": eng.render_targets_timing["marshal_s"],
            "render_and_copy_s": t2 - t1 + eng.render_targets_timing["render_s"],
            "GBps_text_out": n / (t2 - t1 + eng.render_targets_timing["render_s"]) / 1e9}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--flank", type=int, default=100)
    ap.add_argument("--budget", type=int, default=8 << 30)
    ap.add_argument("--compare", type=int, default=0, help="clusters of the single-buffer comparison (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from panfeed_amd.engine import Engine
    res = {"shape": {"clusters": args.clusters, "samples": args.samples, "k": args.k, "flank": args.flank,
                     "budget": args.budget}}
    if args.compare:
        hb, stroi, gen_s = batch(args.compare, args.samples, args.k, args.flank, 10 ** 6)
        eng = Engine(klength=args.k, max_strains=(args.samples + 31) // 32 * 32, stroi=stroi,
                     targets_text_budget=args.budget)
        try:
            one = single_buffer(eng, hb)
            two = streamed(eng, hb, "streamed")
        finally:
            eng.close()
        res["compare"] = {"clusters": args.compare, "generate_pack_s": gen_s, "single_buffer": one, "streamed": two}
        del hb
        print(json.dumps(res["compare"]), flush=True)
    hb, stroi, gen_s = batch(args.clusters, args.samples, args.k, args.flank, 10 ** 6)
    eng = Engine(klength=args.k, max_strains=(args.samples + 31) // 32 * 32, stroi=stroi, targets_text_budget=args.budget)
    try:
        res["full"] = dict(streamed(eng, hb, "streamed"), generate_pack_s=gen_s, instances=int(hb.n_instances))
    finally:
        eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
