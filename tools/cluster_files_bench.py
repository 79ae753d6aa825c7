#!/usr/bin/env python3
"""--multiple-files end to end: run_files(multiple_files=True), plain files, this commit against the parent commit.

Two pangenomes written with panfeed_amd.synth (made once in --files-dir):
(a) 2 000 clusters x 1 000 strains, k = 31, no target strain: two files per cluster, 4 000 small files and 2 000 kmers.tsv
    of one header line;
(b) 64 clusters x 1 000 strains, k = 21, every strain a target: kmers.tsv is nearly all of the output.
Wall seconds of run_files into a fresh directory, median of --runs runs after a warm-up run, with the range, and the
`stages` of the median run (text_s, write_busy_s, submit_s).  Every run's tree is identified by its number of files,
their bytes and one CRC32 over the sorted names and the files' own CRC32s; all runs of both commits must agree.
--parent-root DIR measures the package of another checkout (the parent commit's, built) on the same files in the same
sitting.  Making the files, the measurement and the parent's measurement are three child processes, each under a time
limit of its own; one that fails ends the run.

Writes bench.json and, with --parent-root, parent.json into --out-dir (default profiles/cluster_files/).  Usage:
    python tools/cluster_files_bench.py --files-dir DIR [--shapes a,b] [--runs 5] [--parent-root DIR] [--out-dir DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"files": 900, "measure": 900, "parent": 1100}
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


def tree_id(root):
    """(files, bytes, CRC32 over the sorted relative names and each file's CRC32)"""
    names = []
    for d, _dirs, files in os.walk(root):
        names += [os.path.relpath(os.path.join(d, f), root) for f in files]
    total, crc = 0, 0
    for name in sorted(names):
        file_crc = 0
        with open(os.path.join(root, name), "rb") as fh:
            while True:
                block = fh.read(16 << 20)
                if not block:
                    break
                total += len(block)
                file_crc = zlib.crc32(block, file_crc)
        crc = zlib.crc32(f"{name}:{file_crc}\n".encode(), crc)
    return {"files": len(names), "bytes": total, "crc32": crc}


def timed_runs(args, shape, label):
    from panfeed_amd.pipeline import run_files
    d = os.path.join(args.files_dir, shape)
    with open(os.path.join(d, "done")) as fh:
        made = json.load(fh)
    sh = SHAPES[shape]
    targets = tuple(made["names"]) if sh["all_targets"] else ()
    out = os.path.join(d, "out_" + label)
    runs, tree = [], None
    for i in range(args.runs + 1):
        shutil.rmtree(out, ignore_errors=True)
        t0 = time.perf_counter()
        st = run_files(os.path.join(d, "gene_presence_absence.csv"), os.path.join(d, "gffs"), out, klength=sh["k"],
                       targets=targets, multiple_files=True, batch_clusters=sh["batch_clusters"])
        dt = time.perf_counter() - t0
        assert st["clusters"] == made["clusters"]
        print(f"{label}, shape {shape}: run {i}: {dt:.3f} s  (text {st['stages']['text_s']:.3f}, write "
              f"{st['stages']['write_busy_s']:.3f}, submit {st['stages']['submit_s']:.3f})", flush=True)
        if i == 0 or i == args.runs:            # (the warm-up's and the last run's: the tree is the same every time)
            this = tree_id(out)
            assert tree is None or this == tree, "two runs wrote different trees"
            tree = this
        if i:
            runs.append({"wall_s": dt, "device_cluster_files": st.get("device_cluster_files"),
                         "stages": {k: st["stages"][k] for k in ("text_s", "write_busy_s", "submit_s", "pack_wait_s", "total_s")}})
    shutil.rmtree(out, ignore_errors=True)
    times = [r["wall_s"] for r in runs]
    median = sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2]
    return {"clusters": made["clusters"], "samples": sh["samples"], "k": sh["k"], "targets": len(targets), "stats_bytes": st["bytes"],
            "median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "runs_s": times,
            "median_run": median, "device_cluster_files": runs[-1]["device_cluster_files"], "tree": tree}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files-dir", required=True)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each shape's clusters (a rehearsal)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built: its package is measured on the same files")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "cluster_files"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None, help="(internal) the one step this process runs")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    assert shapes and all(s in SHAPES for s in shapes)
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
    for shape in shapes:
        res[shape] = timed_runs(args, shape, "parent" if parent else "this commit")
        os.makedirs(args.out_dir, exist_ok=True)
        with open(path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    if parent:                                   # both commits' trees, side by side
        with open(os.path.join(args.out_dir, "bench.json")) as fh:
            mine = json.load(fh)
        for shape in shapes:
            assert mine[shape]["tree"] == res[shape]["tree"], f"shape {shape}: the two commits wrote different trees"
            print(f"shape {shape}: trees equal ({res[shape]['tree']}); this commit {mine[shape]['median_s']:.3f} s "
                  f"({mine[shape]['min_s']:.3f} - {mine[shape]['max_s']:.3f}), parent {res[shape]['median_s']:.3f} s "
                  f"({res[shape]['min_s']:.3f} - {res[shape]['max_s']:.3f})", flush=True)


if __name__ == "__main__":
    main()
