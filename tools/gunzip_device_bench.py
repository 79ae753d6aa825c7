#!/usr/bin/env python3
"""Device gunzip of the row filter's .gz inputs against the host's gzip, on the files --gpu-compress writes.

Files: kmers_to_hashes.tsv.gz and kmers.tsv.gz of the tools/gzip_device_bench.py pangenome (run_files with
device_gzip=True; the plain files from a plain run), and the kmers.tsv.gz of one second-pass batch of that tool (the
kmers.tsv stream with device gzip behind a header member, and the plain stream).  Per file:
  - the inflate kernel's time by HIP events (pf_gunzip_device on the file's first 16 MiB of members) and GB/s of text;
  - RowFilter.filter_file wall time on the .gz by the device route and with device_gunzip=False (what --host-gunzip
    runs), median of --runs runs after a warm-up, with the range; the rows of both must be the same bytes;
  - the same on the plain .tsv: the same scan, more bytes over PCIe;
  - the host's zlib inflate rate on the file.
--parent measures the package of another checkout (--package-root, the parent commit's) on the same files: only
filter_file(path), which is all that package has.  The files' sizes and CRC32s are recorded by both, to show they are
the same files.

Writes profiles/gunzip_device/bench.json (parent_filter_file.json with --parent).  Usage:
    python tools/gunzip_device_bench.py [--clusters 300] [--samples 1000] [--targets 4] [--runs 5]
                                        [--stream-clusters 4] [--stream-samples 5000] [--skip-stream]
                                        [--parent --package-root DIR] [--out FILE]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = 64 << 20           # a quarter of this many compressed bytes go to the kernel's figure, at most
SIGNATURE = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0])


def file_id(path):
    crc, n = 0, 0
    with open(path, "rb") as fh:
        while True:
            b = fh.read(1 << 24)
            if not b:
                break
            crc, n = zlib.crc32(b, crc), n + len(b)
    return {"bytes": n, "crc32": crc}


def host_inflate(path):
    t0 = time.perf_counter()
    n = 0
    with gzip.open(path, "rb") as fh:
        while True:
            b = fh.read(1 << 24)
            if not b:
                break
            n += len(b)
    dt = time.perf_counter() - t0
    return {"text_bytes": n, "seconds": dt, "MBps_of_text": n / dt / 1e6}


def keys_of(plain, first_field, matching):
    """keys of the first data row and of one in the middle of the first MiB (matching), or one no row has"""
    if not matching:
        return ["no_such_key"]
    with open(plain, "rb") as fh:
        lines = fh.read(1 << 20).split(b"\n")[1:-1]
    return sorted({ln.split(b"\t")[0 if first_field else -1].decode() for ln in (lines[0], lines[len(lines) // 2])})


def timed_filter(path, first_field, keys, runs, **kw):
    from panfeed_amd.downstream import RowFilter
    times, got, st = [], None, None
    for i in range(runs + 1):
        f = RowFilter(keys, first_field=first_field)
        try:
            t0 = time.perf_counter()
            got = f.filter_file(path, **kw)
            dt = time.perf_counter() - t0
            st = f.stats()
        finally:
            f.close()
        if i:
            times.append(dt)
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times,
            "rows_bytes": len(got[1]), "rows_crc32": zlib.crc32(got[1]), "stats": st}, got


def kernel_time(eng, _lib, path):
    with open(path, "rb") as fh:
        raw = fh.read(SAMPLE // 4)
    cut = raw.rfind(SIGNATURE) if len(raw) == SAMPLE // 4 else len(raw)      # whole members only
    raw = raw[:cut]
    ms_all, n_text = [], 0
    for i in range(6):
        out, n, taken, ms = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_float()
        _lib.check(eng.L.pf_gunzip_device(eng.ctx, raw, len(raw), C.byref(out), C.byref(n), C.byref(taken)))
        eng.L.pf_free_text(out)
        assert taken.value, eng.L.pf_last_error()
        _lib.check(eng.L.pf_gunzip_device_last_ms(eng.ctx, C.byref(ms)))
        n_text = int(n.value)
        if i:
            ms_all.append(float(ms.value))
    ms = statistics.median(ms_all)
    return {"compressed_bytes": len(raw), "text_bytes": n_text, "members": raw.count(SIGNATURE), "kernel_ms": ms, "kernel_ms_runs": ms_all,
            "GBps_of_text": n_text / ms / 1e6}


def per_file(args, eng, _lib, name, gz, plain, first_field, matching):
    keys = keys_of(plain, first_field, matching)
    res = {"file": name, "gz": file_id(gz), "plain": file_id(plain), "first_field": first_field, "keys": keys}
    if args.parent:
        res["filter_file_gz"], _ = timed_filter(gz, first_field, keys, args.runs)
        res["host_zlib_inflate"] = host_inflate(gz)
        return res
    res["inflate_kernel"] = kernel_time(eng, _lib, gz)
    res["filter_file_gz_device"], a = timed_filter(gz, first_field, keys, args.runs, device_gunzip=True)
    res["filter_file_gz_host"], b = timed_filter(gz, first_field, keys, args.runs, device_gunzip=False)
    res["filter_file_plain"], c = timed_filter(plain, first_field, keys, args.runs)
    assert a == b == c, "the three routes' rows differ"
    res["host_zlib_inflate"] = host_inflate(gz)
    res["device_over_host"] = res["filter_file_gz_host"]["median_s"] / res["filter_file_gz_device"]["median_s"]
    return res


def n1_files(args, d):
    from panfeed_amd import synth
    from panfeed_amd.pipeline import run_files
    k, up, down = 31, 100, 100
    cl = synth.generate(args.clusters, args.samples, flank=up)
    csvp, _gffs, _fas = synth.write_pangenome(d, cl, missing_gene_rate=0.0)
    targets = tuple(cl[0].names[:args.targets])
    outs = {}
    for label, kw in (("plain", {}), ("gz", {"device_gzip": True})):
        od = os.path.join(d, "out_" + label)
        run_files(csvp, os.path.join(d, "gffs"), od, klength=k, upstream=up, downstream=down, targets=targets, batch_clusters=64, **kw)
        outs[label] = od
    return outs


def stream_files(args, d):
    """the second-pass batch's kmers.tsv: the device-gzipped stream behind a header member, and the plain stream"""
    from panfeed_amd.engine import Engine
    from panfeed_amd.output import KMERS_TSV_HEADER, MemberGzipWriter
    from tools.targets_stream_scale import batch
    hb, stroi, _gen = batch(args.stream_clusters, args.stream_samples, 21, 100, 10 ** 6)
    paths = {}
    for label, gz in (("plain", False), ("gz", True)):
        paths[label] = os.path.join(d, "second_pass_kmers.tsv" + (".gz" if gz else ""))
        eng = Engine(klength=21, max_strains=(args.stream_samples + 31) // 32 * 32, stroi=stroi, device_gzip=gz)
        w = MemberGzipWriter(paths[label]) if gz else open(paths[label], "wb")
        try:
            w.write(KMERS_TSV_HEADER if gz else KMERS_TSV_HEADER.encode())
            sink = (lambda blk: w.write_members(bytes(blk))) if gz else (lambda blk: w.write(bytes(blk)))
            list(eng.run_batches([hb], prefetch=1, device_text=True, targets_sink=sink))
        finally:
            w.close()
            eng.close()
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clusters", type=int, default=300)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--stream-clusters", type=int, default=4)
    ap.add_argument("--stream-samples", type=int, default=5000)
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--parent", action="store_true", help="measure only filter_file(path): all an earlier package has")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose panfeed_amd package is measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(args.package_root))
    out = args.out or os.path.join(REPO, "profiles", "gunzip_device", "parent_filter_file.json" if args.parent else "bench.json")
    import panfeed_amd
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == os.path.abspath(args.package_root)
    res = {"chunk_bytes": int(_lib.load().pf_gzip_device_chunk_bytes()), "runs": args.runs, "parent": bool(args.parent), "files": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    d = tempfile.mkdtemp()
    try:
        outs = n1_files(args, d)
        eng = None if args.parent else Engine(klength=31, max_strains=32)
        todo = [("n1 kmers_to_hashes", "kmers_to_hashes.tsv", False, True), ("n1 kmers.tsv", "kmers.tsv", True, True)]
        for name, f, first_field, matching in todo:
            res["files"].append(per_file(args, eng, _lib, name, os.path.join(outs["gz"], f + ".gz"), os.path.join(outs["plain"], f),
                                         first_field, matching))
            print(json.dumps(res["files"][-1]), flush=True)
            save()
        if eng:
            eng.close()
        shutil.rmtree(outs["gz"])
        shutil.rmtree(outs["plain"])
        if not args.skip_stream:
            paths = stream_files(args, d)
            eng = None if args.parent else Engine(klength=31, max_strains=32)
            # (four clusters: any one of them is a quarter of the rows, so the key is one that no row has)
            res["files"].append(per_file(args, eng, _lib, "second pass kmers.tsv", paths["gz"], paths["plain"], True, False))
            print(json.dumps(res["files"][-1]), flush=True)
            if eng:
                eng.close()
            save()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
