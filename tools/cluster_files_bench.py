#!/usr/bin/env python3
"""--multiple-files end to end: run_files(multiple_files=True), plain or gzipped files, this commit against the parent commit.

Two pangenomes written with panfeed_amd.synth (made once in --files-dir):
(a) 2 000 clusters x 1 000 strains, k = 31, no target strain: two files per cluster, 4 000 small files and 2 000 kmers.tsv
    of one header line;
(b) 64 clusters x 1 000 strains, k = 21, every strain a target: kmers.tsv is nearly all of the output.
Wall seconds of run_files into a fresh directory, median of --runs runs after a warm-up run, with the range, and the
`stages` of the median run (text_s, write_busy_s, submit_s).  Every run's tree is identified by its number of files,
their bytes and one CRC32 over the sorted names and the files' own CRC32s; all runs of both commits must agree.
--gzip none|host|device (a comma-separated list: one measurement each, in this order): plain files; `compress=True`, the
host's gzip; `device_gzip_clusters=True`, the GPU's (this commit only -- the parent runs `host` in its place, once).  A
gzipped tree is identified twice: as it is (files, bytes, CRC32), and by what it decompresses to (names without `.gz`),
which must be the tree one plain run of the sitting wrote.
--parent-root DIR measures the package of another checkout (the parent commit's, built) on the same files in the same
sitting.  Making the files, the measurement and the parent's measurement are three child processes, each under a time
limit of its own; one that fails ends the run.

Writes bench.json and, with --parent-root, parent.json into --out-dir (default profiles/cluster_files/).  Usage:
    python tools/cluster_files_bench.py --files-dir DIR [--shapes a,b] [--gzip none] [--runs 5] [--parent-root DIR] [--out-dir DIR]
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"files": 900, "measure": 900, "parent": 1100}
GZIP = {"none": {}, "host": {"compress": True}, "device": {"device_gzip_clusters": True}}      # run_files' keywords
# sequence lengths: short genes without flanks, so that the text per cluster -- what this measures -- dominates the input
SYNTH = dict(flank=0, mean_len=300, min_len=100, max_len=900)
SHAPES = {"a": dict(clusters=2000, samples=1000, k=31, all_targets=False, batch_clusters=256),
          "b": dict(clusters=64, samples=1000, k=21, all_targets=True, batch_clusters=256)}


def make_files(args, shape):
    d = os.path.join(args.files_dir, shape)
    done = os.path.join(d, "done")
    if os.path.exists(done):
        return
    from panfeed_amd import synth
    sh = SHAPES[shape]
    os.makedirs(d, exist_ok=True)
    t0 = time.perf_counter()
    cl = synth.generate(int(sh["clusters"] * args.scale) or 1, sh["samples"], **SYNTH)
    print(f"shape {shape}: {len(cl)} clusters generated in {time.perf_counter() - t0:.1f} s", flush=True)
    synth.write_pangenome(d, cl, missing_gene_rate=0.0, workers=min(16, os.cpu_count() or 1))
    print(f"shape {shape}: files written, {time.perf_counter() - t0:.1f} s", flush=True)
    with open(done, "w") as fh:
        fh.write(json.dumps({"clusters": len(cl), "names": cl[0].names}))


def tree_id(root, gunzip=False):
    """(files, bytes, CRC32 over the sorted relative names and each file's CRC32); gunzip: of what the `.gz` files
    decompress to, under their names without `.gz` -- the plain tree's id where they hold its text"""
    names = []
    for d, _dirs, files in os.walk(root):
        names += [os.path.relpath(os.path.join(d, f), root) for f in files]
    assert not gunzip or all(n.endswith(".gz") for n in names)
    total, crc = 0, 0
    for name in sorted(names):
        file_crc = 0
        with (gzip.open if gunzip else open)(os.path.join(root, name), "rb") as fh:
            while True:
                block = fh.read(16 << 20)
                if not block:
                    break
                total += len(block)
                file_crc = zlib.crc32(block, file_crc)
        crc = zlib.crc32(f"{name[:-3] if gunzip else name}:{file_crc}\n".encode(), crc)
    return {"files": len(names), "bytes": total, "crc32": crc}


def timed_runs(args, shape, label, mode="none", n_runs=None):
    """the shape under a gzip mode: a warm-up run and n_runs (default --runs) timed ones; n_runs 0: the warm-up alone, for
    its tree"""
    from panfeed_amd.pipeline import run_files
    n_runs = args.runs if n_runs is None else n_runs
    d = os.path.join(args.files_dir, shape)
    with open(os.path.join(d, "done")) as fh:
        made = json.load(fh)
    sh = SHAPES[shape]
    targets = tuple(made["names"]) if sh["all_targets"] else ()
    out = os.path.join(d, "out_" + label.replace(" ", "_") + "_" + mode)
    runs, tree, text_tree = [], None, None
    for i in range(n_runs + 1):
        shutil.rmtree(out, ignore_errors=True)
        t0 = time.perf_counter()
        st = run_files(os.path.join(d, "gene_presence_absence.csv"), os.path.join(d, "gffs"), out, klength=sh["k"],
                       targets=targets, multiple_files=True, batch_clusters=sh["batch_clusters"], **GZIP[mode])
        dt = time.perf_counter() - t0
        assert st["clusters"] == made["clusters"]
        print(f"{label}, shape {shape}, gzip {mode}: run {i}: {dt:.3f} s  (text {st['stages']['text_s']:.3f}, write "
              f"{st['stages']['write_busy_s']:.3f}, submit {st['stages']['submit_s']:.3f})", flush=True)
        if i == 0 or i == n_runs:               # (the warm-up's and the last run's: the tree is the same every time)
            this = tree_id(out)
            assert tree is None or this == tree, "two runs wrote different trees"
            tree = this
            if mode != "none" and text_tree is None:
                text_tree = tree_id(out, gunzip=True)
        if i:
            runs.append({"wall_s": dt, "device_cluster_files": st.get("device_cluster_files"),
                         "compressed_bytes": st.get("compressed_bytes"),
                         "stages": {k: st["stages"][k] for k in ("text_s", "write_busy_s", "submit_s", "pack_wait_s", "total_s")}})
    shutil.rmtree(out, ignore_errors=True)
    res = {"clusters": made["clusters"], "samples": sh["samples"], "k": sh["k"], "targets": len(targets), "stats_bytes": st["bytes"],
           "gzip": mode, "tree": tree}
    if text_tree is not None:
        res["text_tree"] = text_tree
    if not runs:
        return res
    times = [r["wall_s"] for r in runs]
    median = sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2]
    res.update(median_s=statistics.median(times), min_s=min(times), max_s=max(times), runs_s=times, median_run=median,
               device_cluster_files=runs[-1]["device_cluster_files"], compressed_bytes=runs[-1]["compressed_bytes"])
    return res


def key_of(shape, mode):
    return shape if mode == "none" else f"{shape}_{mode}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files-dir", required=True)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's clusters (a rehearsal)")
    ap.add_argument("--gzip", default="none", help="none, host, device, or a comma-separated list of them")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built: its package is measured on the same files")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "cluster_files"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="(internal) the one step this process runs")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    assert shapes and all(s in SHAPES for s in shapes)
    modes = [m for m in args.gzip.split(",") if m]
    assert modes and all(m in GZIP for m in modes)
    if args.step is None:
        # every step that uses the GPU is a process of its own under its own time limit; a step that fails ends the run
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
        for shape in shapes:
            make_files(args, shape)
        return
    path = os.path.join(args.out_dir, "parent.json" if parent else "bench.json")
    res = {}
    if os.path.exists(path):                     # (the shapes may be measured in sittings of their own)
        with open(path) as fh:
            res = json.load(fh)
    res.update(runs=args.runs, parent=parent, synth=SYNTH)
    label = "parent" if parent else "this commit"
    if parent:                                   # (the parent has no device mode: the host's gzip stands in for it, once)
        modes = list(dict.fromkeys("host" if m == "device" else m for m in modes))

    def save():
        os.makedirs(args.out_dir, exist_ok=True)
        with open(path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    for shape in shapes:
        if not parent and any(m != "none" for m in modes) and "none" not in modes:
            # what the gzipped trees must decompress to: one plain run's tree, not timed
            res[shape + "_plain_tree"] = timed_runs(args, shape, label, "none", n_runs=0)["tree"]
        for mode in modes:
            res[key_of(shape, mode)] = r = timed_runs(args, shape, label, mode)
            if not parent and mode == "none":
                res[shape + "_plain_tree"] = r["tree"]
            save()
    if not parent:
        for shape in shapes:
            for mode in modes:
                if mode != "none":
                    assert res[key_of(shape, mode)]["text_tree"] == res[shape + "_plain_tree"], f"shape {shape}, gzip {mode}: not the plain tree's text"
        return
    # both commits' trees, side by side
    with open(os.path.join(args.out_dir, "bench.json")) as fh:
        mine = json.load(fh)
    for shape in shapes:
        for mode in modes:
            r, m = res[key_of(shape, mode)], mine.get(key_of(shape, mode))
            if mode == "none":
                assert m["tree"] == r["tree"], f"shape {shape}: the two commits wrote different trees"
            else:
                assert r["text_tree"] == mine[shape + "_plain_tree"], f"shape {shape}, gzip {mode}: the parent's tree is not the plain tree's text"
            for who, x in (("this commit", m), ("this commit, device", mine.get(key_of(shape, "device")) if mode == "host" else None), ("parent", r)):
                if x:
                    print(f"shape {shape}, gzip {mode}: {who}: {x['median_s']:.3f} s ({x['min_s']:.3f} - {x['max_s']:.3f}), "
                          f"tree {x['tree']['bytes']} bytes", flush=True)


if __name__ == "__main__":
    main()
