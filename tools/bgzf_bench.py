#!/usr/bin/env python3
"""BGZF on the device against the host's gzip: bgzip'd inputs of the row filter, --bgzf outputs of a run.

Read side.  The three files of tools/gunzip_device_bench.py (the n1 pangenome's kmers_to_hashes.tsv and kmers.tsv, the
kmers.tsv of one second-pass batch) are made as plain text by that tool's own functions and re-written here as BGZF, as
`bgzip` cuts them: members of 65 280 bytes of text, zlib level 6, then the end marker (a maker of this tool's own, from the
SAM specification -- no bgzip needed).  Per file:
  - the new inflate kernel's time by HIP events (pf_gunzip_device_bgzf on the file's first 16 MiB) and GB/s of text;
  - RowFilter.filter_file wall time by the device route and with device_gunzip=False, median of --runs runs after a
    warm-up, with the range; the rows of both must be the same bytes; the host's zlib inflate rate.
--parent measures the package of another checkout (--package-root, the parent commit's) on the same files: only
filter_file(path) -- there a BGZF file goes the host's way.  Sizes and CRC32s are recorded by both.

Write side (--write): run_files over the n1 pangenome with device_gzip and with device_gzip + bgzf, median of --runs after
a warm-up, the three files' sizes and their ratio; with --parent only device_gzip, which is all that package has.

Writes profiles/bgzf/bench.json (parent.json with --parent).  Usage:
    python tools/bgzf_bench.py [--clusters 300] [--samples 1000] [--targets 4] [--runs 5] [--skip-stream] [--write]
                               [--parent --package-root DIR] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import gunzip_device_bench as gb  # noqa: E402

BLOCK, LEVEL = 65280, 6
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_bgzf(plain, path):
    """`plain` as bgzip writes it; -> members written (the end marker among them)"""
    n = 0
    with open(plain, "rb") as src, open(path, "wb") as dst:
        while True:
            text = src.read(BLOCK)
            if not text:
                break
            z = zlib.compressobj(LEVEL, zlib.DEFLATED, -15)
            body = z.compress(text) + z.flush()
            dst.write(bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H2sHH", 6, b"BC", 2, 18 + len(body) + 8 - 1) + body
                      + struct.pack("<II", zlib.crc32(text), len(text)))
            n += 1
        dst.write(EOF)
    return n + 1


def kernel_time(eng, _lib, path):
    """whole members of the file's first 16 MiB through pf_gunzip_device_bgzf: the inflate launches by HIP events"""
    with open(path, "rb") as fh:
        raw = fh.read(gb.SAMPLE // 4)
    at = members = 0
    while at + 18 <= len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        if at + size > len(raw):
            break
        at, members = at + size, members + 1
    raw = raw[:at]
    ms_all, n_text = [], 0
    for i in range(6):
        out, n, taken, ms = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_float()
        _lib.check(eng.L.pf_gunzip_device_bgzf(eng.ctx, raw, len(raw), C.byref(out), C.byref(n), C.byref(taken)))
        eng.L.pf_free_text(out)
        assert taken.value, eng.L.pf_last_error()
        _lib.check(eng.L.pf_gunzip_device_last_ms(eng.ctx, C.byref(ms)))
        n_text = int(n.value)
        if i:
            ms_all.append(float(ms.value))
    ms = statistics.median(ms_all)
    return {"compressed_bytes": len(raw), "text_bytes": n_text, "members": members, "kernel_ms": ms, "kernel_ms_runs": ms_all,
            "GBps_of_text": n_text / ms / 1e6}


def per_file(args, eng, _lib, name, plain, first_field, matching):
    gz = plain + ".bgzf.gz"
    members = write_bgzf(plain, gz)
    keys = gb.keys_of(plain, first_field, matching)
    res = {"file": name, "gz": gb.file_id(gz), "plain": gb.file_id(plain), "members": members, "first_field": first_field, "keys": keys}
    if args.parent:
        res["filter_file_gz"], _ = gb.timed_filter(gz, first_field, keys, args.runs)
    else:
        res["inflate_kernel"] = kernel_time(eng, _lib, gz)
        res["filter_file_gz_device"], a = gb.timed_filter(gz, first_field, keys, args.runs, device_gunzip=True)
        res["filter_file_gz_auto"], b = gb.timed_filter(gz, first_field, keys, args.runs)
        res["filter_file_gz_host"], c = gb.timed_filter(gz, first_field, keys, args.runs, device_gunzip=False)
        assert a == b == c, "the routes' rows differ"
        assert res["filter_file_gz_auto"]["stats"]["gunzip_fallbacks"] == 0
        res["device_over_host"] = res["filter_file_gz_host"]["median_s"] / res["filter_file_gz_device"]["median_s"]
    res["host_zlib_inflate"] = gb.host_inflate(gz)
    os.remove(gz)
    return res


def plain_n1(args, d):
    """the n1 pangenome's plain files, and what run_files needs to run it again: (csv, gffs, run_files keywords, output)"""
    from panfeed_amd import synth
    from panfeed_amd.pipeline import run_files
    k, up, down = 31, 100, 100
    cl = synth.generate(args.clusters, args.samples, flank=up)
    csvp, _gffs, _fas = synth.write_pangenome(d, cl, missing_gene_rate=0.0)
    kw = dict(klength=k, upstream=up, downstream=down, targets=tuple(cl[0].names[:args.targets]), batch_clusters=64)
    od = os.path.join(d, "out_plain")
    run_files(csvp, os.path.join(d, "gffs"), od, **kw)
    return csvp, os.path.join(d, "gffs"), kw, od


def write_side(args, csvp, gffs, kw, d):
    from panfeed_amd.pipeline import run_files
    res = {}
    for label, more in (("gpu_compress", {"device_gzip": True}),) + (() if args.parent else (("gpu_compress_bgzf", {"device_gzip": True, "bgzf": True}),)):
        times, sizes = [], {}
        for i in range(args.runs + 1):
            od = os.path.join(d, f"out_{label}_{i}")
            t0 = time.perf_counter()
            run_files(csvp, gffs, od, **kw, **more)
            dt = time.perf_counter() - t0
            if i:
                times.append(dt)
            sizes = {f: os.path.getsize(os.path.join(od, f)) for f in sorted(os.listdir(od))}
            shutil.rmtree(od)
        res[label] = {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times, "file_bytes": sizes,
                      "total_bytes": sum(sizes.values())}
    if not args.parent:
        res["bgzf_over_plain_members_bytes"] = res["gpu_compress_bgzf"]["total_bytes"] / res["gpu_compress"]["total_bytes"]
        res["bgzf_over_plain_members_time"] = res["gpu_compress_bgzf"]["median_s"] / res["gpu_compress"]["median_s"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--stream-clusters", type=int, default=4)
    ap.add_argument("--stream-samples", type=int, default=5000)
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-read", action="store_true")
    ap.add_argument("--write", action="store_true", help="measure the write side too")
    ap.add_argument("--parent", action="store_true", help="measure only what an earlier package has")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose panfeed_amd package is measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    out = args.out or os.path.join(REPO, "profiles", "bgzf", "parent.json" if args.parent else "bench.json")
    import panfeed_amd
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == os.path.abspath(args.package_root)
    res = {"block_bytes": BLOCK, "level": LEVEL, "runs": args.runs, "parent": bool(args.parent), "files": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    d = tempfile.mkdtemp()
    try:
        csvp, gffs, kw, od = plain_n1(args, d)
        if not args.skip_read:
            eng = None if args.parent else Engine(klength=31, max_strains=32)
            for name, f, first_field, matching in (("n1 kmers_to_hashes", "kmers_to_hashes.tsv", False, True), ("n1 kmers.tsv", "kmers.tsv", True, True)):
                res["files"].append(per_file(args, eng, _lib, name, os.path.join(od, f), first_field, matching))
                print(json.dumps(res["files"][-1]), flush=True)
                save()
            if eng:
                eng.close()
        shutil.rmtree(od)
        if args.write:
            res["write_side"] = write_side(args, csvp, gffs, kw, d)
            print(json.dumps(res["write_side"]), flush=True)
            save()
        if not args.skip_stream and not args.skip_read:
            # the plain stream of one second-pass batch, as tools/gunzip_device_bench.py makes it
            from panfeed_amd.output import KMERS_TSV_HEADER
            from tools.targets_stream_scale import batch
            hb, stroi, _gen = batch(args.stream_clusters, args.stream_samples, 21, 100, 10 ** 6)
            plain = os.path.join(d, "second_pass_kmers.tsv")
            eng = Engine(klength=21, max_strains=(args.stream_samples + 31) // 32 * 32, stroi=stroi)
            with open(plain, "wb") as w:
                w.write(KMERS_TSV_HEADER.encode())
                list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=lambda blk: w.write(bytes(blk))))
            eng.close()
            eng = None if args.parent else Engine(klength=31, max_strains=32)
            res["files"].append(per_file(args, eng, _lib, "second pass kmers.tsv", plain, True, False))
            print(json.dumps(res["files"][-1]), flush=True)
            if eng:
                eng.close()
            save()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
