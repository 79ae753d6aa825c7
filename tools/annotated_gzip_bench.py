#!/usr/bin/env python3
"""The annotated table compressed at both ends: panfeed-get-kmers --gz-output against its plain output, and panfeed-plot's
scan of the .gz by the device route against the host's gzip and against the parent commit.

Files (made once in --files-dir): the second-pass-shaped tables of tools/get_kmers_join_bench.py (4 clusters x 250 strains,
kmers.tsv of 887 445 rows) and the one-cluster table of tools/plot_bench.py (5 000 strains x ~1 200 positions, 6.3 M rows),
plain and as a .gz of device-made members behind a header member (pf_gzip_device, which the parent commit has too).
(a) get_kmers, wall time to a file, median of --runs runs after a warm-up with the range: plain output (`out` a file) and
    --gz-output; the .gz file's bytes beside zlib level 1 and level 9 over the same cuts -- the members' own ISIZEs --,
    the yardstick of profiles/gzip_device/README.md; the file must inflate to the plain output.
(b) plot, GridBuilder.scan_file + finish on a fresh builder, the same statistic: the plain table, the .gz by the device
    route (device_gunzip=True), the .gz with device_gunzip=False (what --host-gunzip runs); clusters, records and lines of
    the three must agree.
--parent-root DIR measures the package of another checkout (the parent commit's, built) on the same files: get_kmers to a
plain file and scan_file(path) on the .gz, which is all that package has.  The files' sizes and CRC32s are recorded by
both.  Making the files, the measurement and the parent's measurement are three child processes, each under a time limit
of its own; one that fails ends the run.

Writes bench.json and, with --parent-root, parent.json into --out-dir (default profiles/annotated_gzip/).  Usage:
    python tools/annotated_gzip_bench.py --files-dir DIR [--runs 5] [--parent-root DIR] [--out-dir DIR]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0])
PLOT_STRAINS = 5000
STEP_LIMIT_S = {"files": 900, "measure": 900, "parent": 600}


def _summary(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times}


def make_files(args):
    from tools.get_kmers_join_bench import make_files as join_files
    from tools.plot_bench import make_table
    join_files(args)                                     # (its own `done` mark)
    done = os.path.join(args.files_dir, "plot_done")
    if os.path.exists(done):
        return
    from panfeed_amd import _lib
    from panfeed_amd.engine import Engine
    from panfeed_amd.output import MemberGzipWriter
    plain = os.path.join(args.files_dir, "plot_table.tsv")
    rows = make_table(plain, 1, 1.0)
    eng = Engine(klength=31, max_strains=32)
    try:
        with open(plain, "rb") as fh, MemberGzipWriter(plain + ".gz") as w:
            w.write(fh.readline())
            carry = b""
            while True:
                block = fh.read(64 << 20)
                data = carry + block
                cut = len(data) if not block else data.rfind(b"\n") + 1
                if cut:
                    out, n = C.c_void_p(), C.c_uint64()
                    _lib.check(eng.L.pf_gzip_device(eng.ctx, data[:cut], cut, 0, C.byref(out), C.byref(n)))
                    w.write_members(C.string_at(out, n.value))
                    eng.L.pf_free_text(out)
                carry = data[cut:]
                if not block:
                    break
    finally:
        eng.close()
    with open(done, "w") as fh:
        fh.write(str(rows))


def zlib_on_members(gz_path):
    """the file's members, their text bytes, and what zlib makes of the same pieces of text at level 1 and 9 (gzip frames)"""
    with open(gz_path, "rb") as fh:
        raw = fh.read()
    text = gzip.decompress(raw)
    starts, at = [], raw.find(SIGNATURE)
    while at >= 0:
        starts.append(at)
        at = raw.find(SIGNATURE, at + 1)
    ends = starts[1:] + [len(raw)]
    isize = [int.from_bytes(raw[e - 4:e], "little") for e in ends]
    assert sum(isize) == len(text)
    totals, at = {1: 0, 9: 0}, 0
    for n in isize:
        for level in totals:
            z = zlib.compressobj(level, zlib.DEFLATED, 31)
            totals[level] += len(z.compress(text[at:at + n])) + len(z.flush())
        at += n
    return {"members": len(isize), "short_members": sum(1 for n in isize if n < max(isize)), "text_bytes": len(text),
            "text_crc32": zlib.crc32(text), "file_bytes": len(raw), "zlib1_on_cuts_bytes": totals[1], "zlib9_on_cuts_bytes": totals[9],
            "file_over_zlib1": len(raw) / totals[1], "ratio": len(text) / len(raw)}


def timed_get_kmers(args, file_id, gz, label):
    from panfeed_amd import downstream
    d = args.files_dir
    out_path = os.path.join(d, "annotated.tsv" + (".gz" if gz else ""))
    argv = ["-a", os.path.join(d, "assoc.tsv"), "-p", os.path.join(d, "out_gz", "kmers_to_hashes.tsv.gz"),
            "-k", os.path.join(d, "out_gz", "kmers.tsv.gz"), "-t", "0.01"]
    times = []
    for i in range(args.runs + 1):
        t0 = time.perf_counter()
        if gz:
            rc = downstream.get_kmers(argv + ["--gz-output", out_path])
        else:
            with open(out_path, "w", encoding="utf-8") as out:
                rc = downstream.get_kmers(argv, out=out)
        dt = time.perf_counter() - t0
        assert rc == 0
        if i:
            times.append(dt)
        print(f"{label}: run {i}: {dt:.3f} s", flush=True)
    kj = downstream.KmerJoin
    stats = dict(kj.last_stats, device_bunches=kj.device_bunches, host_bunches=kj.host_bunches, host_runs=kj.host_runs)
    return dict(_summary(times), output=file_id(out_path), stats=stats), out_path


def timed_scan(args, path, label, **kw):
    from panfeed_amd import plot as P
    strains = [f"s{i}" for i in range(PLOT_STRAINS)]
    columns = P.table_columns(path, "lrt-pvalue")
    times, found = [], None
    for i in range(args.runs + 1):
        gb = P.GridBuilder(strains, columns)
        try:
            t0 = time.perf_counter()
            gb.scan_file(path, **kw)
            gb.finish()
            dt = time.perf_counter() - t0
            st = gb.stats()
            found = {"clusters": len(gb.clusters), "pvalue_texts": len(gb.pvalue_texts), "records": gb.n_records, "lines": st["lines"],
                     "min": [int(x) for x in gb.min], "max": [int(x) for x in gb.max]}
        finally:
            gb.close()
        if i:
            times.append(dt)
        print(f"{label}: run {i}: {dt:.3f} s", flush=True)
    return dict(_summary(times), found=found, stats=st)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files-dir", required=True)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--pass-every", type=int, default=25)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built: its package is measured on the same files")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "annotated_gzip"))
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
    sys.path.insert(0, REPO)                             # (tools.*, behind the package's root)
    sys.path.insert(0, root)
    import panfeed_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(panfeed_amd.__file__))) == root
    from tools.get_kmers_join_bench import file_id
    if args.step == "files":
        make_files(args)
        return
    d = args.files_dir
    out = os.path.join(args.out_dir, "parent.json" if args.parent else "bench.json")
    plot_plain, plot_gz = os.path.join(d, "plot_table.tsv"), os.path.join(d, "plot_table.tsv.gz")
    res = {"runs": args.runs, "parent": bool(args.parent),
           "inputs": {"kmers.tsv.gz": file_id(os.path.join(d, "out_gz", "kmers.tsv.gz")),
                      "kmers_to_hashes.tsv.gz": file_id(os.path.join(d, "out_gz", "kmers_to_hashes.tsv.gz")),
                      "plot_table.tsv": file_id(plot_plain), "plot_table.tsv.gz": file_id(plot_gz)}}

    def save():
        os.makedirs(args.out_dir, exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    res["get_kmers_plain"], plain_out = timed_get_kmers(args, file_id, False, "get_kmers, plain output")
    save()
    if args.parent:
        res["plot_scan_gz"] = timed_scan(args, plot_gz, "parent, plot scan of the .gz")
        save()
        print(json.dumps(res))
        return
    res["get_kmers_gz"], gz_out = timed_get_kmers(args, file_id, True, "get_kmers, --gz-output")
    res["gz_file"] = zlib_on_members(gz_out)
    assert res["gz_file"]["text_bytes"] == res["get_kmers_plain"]["output"]["bytes"]
    assert res["gz_file"]["text_crc32"] == res["get_kmers_plain"]["output"]["crc32"], "the .gz does not inflate to the plain output"
    res["gz_over_plain"] = res["get_kmers_gz"]["median_s"] / res["get_kmers_plain"]["median_s"]
    save()
    res["plot_scan_plain"] = timed_scan(args, plot_plain, "plot scan, plain")
    res["plot_scan_gz_device"] = timed_scan(args, plot_gz, "plot scan, .gz, device route", device_gunzip=True)
    res["plot_scan_gz_host"] = timed_scan(args, plot_gz, "plot scan, .gz, host gunzip", device_gunzip=False)
    founds = [res[k]["found"] for k in ("plot_scan_plain", "plot_scan_gz_device", "plot_scan_gz_host")]
    assert founds[0] == founds[1] == founds[2], "the three routes' grids differ"
    res["host_over_device"] = res["plot_scan_gz_host"]["median_s"] / res["plot_scan_gz_device"]["median_s"]
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
