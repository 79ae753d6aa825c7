#!/usr/bin/env python3
"""Device gzip (--gpu-compress) against the host's gzip and against zlib on the device's own chunk cuts.

Part 1, the tools/n1_bench.py pangenome (clusters x samples, a few target strains): per output file the text bytes; bytes
and seconds of the host path (pf_gzip_members, level 9, as `--compress` runs it); bytes of zlib level 1 and level 9 over the
device's chunk cuts (and level 1 over 16 / 32 / 64 KiB cuts: what the chunk size costs); the device's bytes, its kernel time by HIP events as GB/s of text, and its wall time with upload and
D2H; then run_files end to end -- plain, compress=True, device_gzip=True -- median of --runs runs after a warm-up.
Part 2, one BASELINE configs[4]-shaped second-pass batch (tools/targets_stream_scale.py's: every strain a target): the
kmers.tsv stream with and without device gzip into a counting sink, and the host path's rate on a sample of that text.  Both
streams run once more, untimed, into a sink that inflates the members: the text behind them must be the plain stream's.

--level: the encoder's effort levels to measure, one or both in one session (1: flags 0; 2: PF_GZ_DEEP).  The first one
given fills the fields above as before; every level's device bytes and times stand under "levels", and zlib 4 and 6 on the
same cuts beside 1 and 9.  --skip-e2e leaves the run_files legs out (a kernel-time-only run, as for a parent commit).

Writes one JSON file into profiles/gzip_device/.  Usage:
    python tools/gzip_device_bench.py [--clusters 300] [--samples 1000] [--targets 4] [--runs 5] [--level 1 2]
                                      [--stream-clusters 4] [--stream-samples 5000] [--out profiles/gzip_device/bench.json]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SAMPLE = 64 << 20           # bytes of a file's text the per-file figures are taken on


def host_gzip(L, _lib, text):
    out, n = C.c_void_p(), C.c_uint64()
    t0 = time.perf_counter()
    _lib.check(L.pf_gzip_members(text, len(text), 9, 4 << 20, C.byref(out), C.byref(n)))
    dt = time.perf_counter() - t0
    L.pf_free_text(out)
    return int(n.value), dt


def zlib_on_cuts(text, cut, level):
    total = 0
    for at in range(0, len(text), cut):
        z = zlib.compressobj(level, zlib.DEFLATED, 31)
        total += len(z.compress(text[at:at + cut])) + len(z.flush())
    return total


LEVEL_FLAGS = {1: 0, 2: 16}          # (2: PF_GZ_DEEP)
LEVELS = [1]                         # --level


def level_kw(level):
    """run_files' / Engine's argument for a level; none for 1, so that the tool also runs against an older tree"""
    return {} if level == 1 else {"device_gzip_level": level}


def device_gzip(eng, _lib, text, level=1):
    out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    t0 = time.perf_counter()
    _lib.check(eng.L.pf_gzip_device(eng.ctx, text, len(text), LEVEL_FLAGS[level], C.byref(out), C.byref(n)))
    dt = time.perf_counter() - t0
    _lib.check(eng.L.pf_gzip_device_last_ms(eng.ctx, C.byref(ms)))
    members = C.string_at(out, n.value)
    eng.L.pf_free_text(out)
    assert zlib.decompressobj(31).decompress(members)[:64] == text[:64]
    return int(n.value), float(ms.value), dt


def device_level(eng, _lib, text, level):
    """bytes, kernel ms (median and the runs: their range is the run-to-run spread) and wall seconds of one level"""
    device_gzip(eng, _lib, text[:1 << 20], level)               # warm-up: buffers, first launch
    runs = [device_gzip(eng, _lib, text, level) for _ in range(5)]
    ms = statistics.median(r[1] for r in runs)
    return {"device_bytes": runs[0][0], "device_kernel_ms": ms, "device_kernel_ms_runs": [r[1] for r in runs],
            "device_kernel_GBps": len(text) / ms / 1e6, "device_wall_s": statistics.median(r[2] for r in runs),
            "ratio_device": len(text) / runs[0][0]}


def per_file(eng, _lib, name, text):
    cut = int(eng.L.pf_gzip_device_chunk_bytes())
    text = text[:SAMPLE]
    hb, hs = host_gzip(eng.L, _lib, text)
    levels = {str(level): device_level(eng, _lib, text, level) for level in LEVELS}
    first = levels[str(LEVELS[0])]
    db, ms, wall = first["device_bytes"], first["device_kernel_ms"], first["device_wall_s"]
    z1, z9 = zlib_on_cuts(text, cut, 1), zlib_on_cuts(text, cut, 9)
    z4, z6 = zlib_on_cuts(text, cut, 4), zlib_on_cuts(text, cut, 6)
    by_cut = {str(c): zlib_on_cuts(text, c, 1) for c in (16 << 10, 32 << 10, 64 << 10)}     # what the chunk size costs
    return {"file": name, "zlib1_bytes_by_cut": by_cut, "text_bytes": len(text), "host_level9_bytes": hb, "host_level9_s": hs,
            "host_level9_MBps": len(text) / hs / 1e6, "zlib1_on_cuts_bytes": z1, "zlib9_on_cuts_bytes": z9,
            "device_bytes": db, "device_over_zlib1": db / z1, "ratio_device": len(text) / db, "ratio_zlib1": len(text) / z1,
            "ratio_host_level9": len(text) / hb, "device_kernel_ms": ms, "device_kernel_GBps": len(text) / ms / 1e6,
            "device_wall_s": wall, "zlib4_on_cuts_bytes": z4, "zlib6_on_cuts_bytes": z6, "levels": levels}


def part1(args, res):
    from panfeed_amd import _lib, synth
    from panfeed_amd.engine import Engine
    from panfeed_amd.pipeline import run_files
    k, up, down = 31, 100, 100
    cl = synth.generate(args.clusters, args.samples, flank=up)
    d = tempfile.mkdtemp()
    csvp, _gffs, _fas = synth.write_pangenome(d, cl, missing_gene_rate=0.0)
    targets = tuple(cl[0].names[:args.targets])

    def run(**kw):
        od = os.path.join(tempfile.mkdtemp(), "panfeed")
        t0 = time.perf_counter()
        st = run_files(csvp, os.path.join(d, "gffs"), od, klength=k, upstream=up, downstream=down, targets=targets,
                       batch_clusters=64, **kw)
        return od, st, time.perf_counter() - t0
    od, st, _ = run()
    eng = Engine(klength=k, max_strains=32)
    files = []
    for f in ("kmers_to_hashes.tsv", "hashes_to_patterns.tsv", "kmers.tsv"):
        with open(os.path.join(od, f), "rb") as fh:
            files.append(per_file(eng, _lib, f, fh.read()))
        print(json.dumps(files[-1]), flush=True)
    eng.close()
    shutil.rmtree(os.path.dirname(od))
    e2e = {}
    legs = [("plain", {}), ("compress", {"compress": True})]
    legs += [("device_gzip" if level == LEVELS[0] else f"device_gzip_level{level}", dict(device_gzip=True, **level_kw(level)))
             for level in LEVELS]
    for label, kw in ([] if args.skip_e2e else legs):
        times, size = [], 0
        for i in range(args.runs + 1):
            od, st, dt = run(**kw)
            size = sum(os.path.getsize(os.path.join(od, f)) for f in os.listdir(od))
            shutil.rmtree(os.path.dirname(od))
            if i:
                times.append(dt)
        e2e[label] = {"median_s": statistics.median(times), "runs_s": times, "file_bytes": size, "text_bytes": st["bytes"]}
        print(label, json.dumps(e2e[label]), flush=True)
    res["n1"] = {"clusters": args.clusters, "samples": args.samples, "targets": args.targets, "files": files, "run_files": e2e}
    shutil.rmtree(d)


class _Decoded:
    """a sink's running CRC32 and size of the text it was handed: as text, or as gzip members it inflates"""

    def __init__(self, members):
        self.members, self.crc, self.n = members, 0, 0

    def __call__(self, blk):
        raw = bytes(blk)
        while raw:
            if self.members:
                d = zlib.decompressobj(31)
                text, raw = d.decompress(raw), d.unused_data
                assert d.eof
            else:
                text, raw = raw, b""
            self.crc = zlib.crc32(text, self.crc)
            self.n += len(text)


def part2(args, res):
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    from tools.targets_stream_scale import batch
    hb, stroi, _gen = batch(args.stream_clusters, args.stream_samples, 21, 100, 10 ** 6)
    out = {"clusters": args.stream_clusters, "samples": args.stream_samples}
    sample = bytearray()
    decoded = {}
    # timed with a counting sink first; then once more each way with a sink that inflates the blocks, untimed: the text
    # behind the members must be the plain stream's (blocks past a range's first included: the batch is one long range)
    flags = {} if LEVELS[0] == 1 else {"device_gzip_flags": LEVEL_FLAGS[LEVELS[0]]}      # (the stream runs at the first level given)
    for label, gz, check in (("plain", False, False), ("device_gzip", True, False), ("plain", False, True), ("device_gzip", True, True)):
        eng = Engine(klength=21, max_strains=(args.stream_samples + 31) // 32 * 32, stroi=stroi, device_gzip=gz, **(flags if gz else {}))
        n = [0]

        def count(blk):
            n[0] += len(blk)
            if not gz and len(sample) < SAMPLE:
                sample.extend(blk[:SAMPLE - len(sample)])
        sink = _Decoded(gz) if check else count
        try:
            o = list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=sink))[0]
            if check:
                decoded[label] = (sink.crc, sink.n)
                continue
            s = eng.render_targets_timing["render_s"]
            out[label] = {"text_bytes": o.stats["kmers_tsv_streamed"], "bytes_to_the_sink": n[0], "stream_s": s,
                          "GBps_of_text": o.stats["kmers_tsv_streamed"] / s / 1e9, "ranges": o.stats["kmers_tsv_ranges"],
                          "peak_device_bytes": o.stats["kmers_tsv_peak_device_bytes"]}
            if gz:
                out["kmers_tsv_sample"] = per_file(eng, _lib, "kmers.tsv (second pass)", bytes(sample))
        finally:
            eng.close()
        print(label, json.dumps(out[label]), flush=True)
    assert decoded["plain"] == decoded["device_gzip"] and decoded["plain"][1] == out["plain"]["text_bytes"], decoded
    out["members_decode_to_the_plain_stream"] = {"crc32": decoded["plain"][0], "text_bytes": decoded["plain"][1]}
    res["second_pass_batch"] = out


def _save(args, res):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--stream-clusters", type=int, default=4)
    ap.add_argument("--stream-samples", type=int, default=5000)
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true", help="leave the run_files legs out")
    ap.add_argument("--level", type=int, nargs="+", choices=(1, 2), default=[1],
                    help="the encoder's effort levels to measure (default: 1)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gzip_device", "bench.json"))
    args = ap.parse_args()
    LEVELS[:] = list(dict.fromkeys(args.level))
    from panfeed_amd import _lib
    res = {"chunk_bytes": int(_lib.load().pf_gzip_device_chunk_bytes()), "flags": LEVEL_FLAGS[LEVELS[0]], "levels": LEVELS}
    part1(args, res)
    _save(args, res)
    if not args.skip_stream:
        part2(args, res)
        _save(args, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
