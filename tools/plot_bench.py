#!/usr/bin/env python3
"""panfeed-plot's grid pass on synthetic annotated tables shaped like the second pass of configs[4]:
one cluster of 5 000 strains x ~1 200 positions, and 64 such clusters (rows at a given density).

Prints one JSON line per shape: rows/s and device ms of the grid pass (stream + grids), host ms of the strain ordering
and hybrid normalisation, rendering seconds per figure.  `--cpu-pivots` times instead the reference's semantics on the
CPU for one cluster (its pivot_table with the Python aggfunc, plot.py:283-285, and the builtin-max pivot, :261-264),
on a slice of `--pivot-strains` strains.

Usage: python tools/plot_bench.py [--clusters 1 64] [--density 1 0.1] [--render 1]
       python tools/plot_bench.py --cpu-pivots [--pivot-strains 1000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STRAINS, POSITIONS = 5000, 1200


def make_table(path, n_clusters, density, seed=1, strains=STRAINS):
    """cluster, k-mer, lrt-pvalue, strain, gene_start, strand; a row per (strain, position) kept at `density`"""
    rng = np.random.default_rng(seed)
    pv = np.array([f"{x:.2E}" for x in 10 ** rng.uniform(-12, 0, 4000)] + [""])
    rows = 0
    with open(path, "w") as fh:
        fh.write("cluster\tk-mer\tlrt-pvalue\tstrain\tgene_start\tstrand\n")
        for c in range(n_clusters):
            width = POSITIONS + int(rng.integers(-100, 100))
            s, x = np.meshgrid(np.arange(strains), np.arange(width) - 100, indexing="ij")
            s, x = s.ravel(), x.ravel()
            if density < 1:
                keep = rng.random(len(s)) < density
                s, x = s[keep], x[keep]
            n = len(s)
            kmer = np.array(["ACGTACGTACGTACGTACGTACGTACGTACG", "TGCATGCATGCATGCATGCATGCATGCATGC",
                             "GGCATTACGATCAGCTAGCATCGACTAGCAN"])[rng.integers(0, 3, n)]
            cols = [np.full(n, f"group_{c:06d}"), kmer, pv[rng.integers(0, len(pv), n)], np.char.add("s", s.astype(str)),
                    x.astype(str), np.where(rng.random(n) < 0.5, "-1", "1")]
            lines = cols[0]
            for col in cols[1:]:
                lines = np.char.add(np.char.add(lines, "\t"), col)
            fh.write("\n".join(lines.tolist()) + "\n")
            rows += n
    return rows


def gpu_bench(n_clusters, density, render):
    import pandas as pd  # noqa: F401

    from panfeed_amd import plot as P
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "annotated.tsv")
        rows = make_table(path, n_clusters, density)
        size = os.path.getsize(path)
        strains = [f"s{i}" for i in range(STRAINS)]
        ph = P.Phenotype(strains, False, None, False)
        t0 = time.perf_counter()
        gb = P.GridBuilder(strains, P.table_columns(path, "lrt-pvalue"))
        gb.scan_file(path)
        gb.finish()
        gb.set_significance(P.significance_of(gb.pvalue_texts))
        t_scan = time.perf_counter() - t0
        ids_of = {s: i for i, s in enumerate(strains)}
        order = sorted(range(len(gb.clusters)), key=lambda i: gb.clusters[i])
        t_grid = t_host = 0.0
        figs = []
        budget = P.GRID_BUDGET // 16
        i = 0
        while i < len(order):
            batch, cells = [], 0
            while i < len(order) and (not batch or cells + gb.width(order[i]) * STRAINS <= budget):
                batch.append(order[i])
                cells += gb.width(order[i]) * STRAINS
                i += 1
            t0 = time.perf_counter()
            grids = gb.grids(batch)
            t_grid += time.perf_counter() - t0
            for c, (key, cnt) in zip(batch, grids):
                t0 = time.perf_counter()
                f = P._figure(gb.clusters[c], key, cnt, ph, strains, ids_of, gb.min[c], gb.max[c], 1.0, 1e-10, 0.0, 200,
                              False)
                t_host += time.perf_counter() - t0
                if len(figs) < render:
                    figs.append(f)
        st = gb.stats()
        gb.close()
        t_render = None
        if figs:
            import matplotlib
            matplotlib.use("Agg")
            args = P.get_options(["-k", path, "-p", "x", "--output-directory", d])
            cmap1, cmap2 = P._colormaps()
            t0 = time.perf_counter()
            for f in figs:
                P.render(f, args, cmap1, cmap2)
            t_render = (time.perf_counter() - t0) / (3 * len(figs))
    return {"shape": f"{n_clusters} x {STRAINS} strains x ~{POSITIONS} positions, density {density}", "rows": rows,
            "bytes": size, "records": st["records"], "grid_pass_s": round(t_scan + t_grid, 3),
            "rows_per_s": round(rows / (t_scan + t_grid)), "device_ms": round(st["device_ms"], 1),
            "host_order_normalise_ms_per_cluster": round(1000 * t_host / max(1, len(order)), 1),
            "render_s_per_figure": None if t_render is None else round(t_render, 2)}


def handle_paralogs(x):                 # the reference's aggfunc (plot.py:226-229), restated for timing
    if len(x) > 1:
        return 99
    return x


def cpu_pivots(n_strains):
    import pandas as pd
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "annotated.tsv")
        make_table(path, 1, 1.0, strains=n_strains)
        k = pd.read_csv(path, sep="\t")
    k["significance"] = -np.log10(k["lrt-pvalue"])
    k["scalar"] = k["k-mer"].str[0].map({"A": 0, "G": 1, "T": 2, "C": 3})
    cells = k["strain"].nunique() * k["gene_start"].nunique()
    t0 = time.perf_counter()
    k.pivot_table(index="strain", columns="gene_start", values="significance", aggfunc="max")
    t_max = time.perf_counter() - t0
    t0 = time.perf_counter()
    k.pivot_table(index="strain", columns="gene_start", values="scalar", aggfunc=handle_paralogs)
    t_py = time.perf_counter() - t0
    return {"cpu_pivots": f"{n_strains} strains x ~{POSITIONS} positions", "cells": int(cells),
            "max_pivot_s_per_Mcell": round(t_max / cells * 1e6, 3), "aggfunc_pivot_s_per_Mcell": round(t_py / cells * 1e6, 2),
            "pandas": pd.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--density", type=float, nargs="+", default=[1.0, 0.1])
    ap.add_argument("--render", type=int, default=1, help="clusters whose three figures are rendered and timed")
    ap.add_argument("--cpu-pivots", action="store_true")
    ap.add_argument("--pivot-strains", type=int, default=1000)
    a = ap.parse_args()
    if a.cpu_pivots:
        print(json.dumps(cpu_pivots(a.pivot_strains)))
        return
    for n, dens in zip(a.clusters, a.density):
        print(json.dumps(gpu_bench(n, dens, a.render)), flush=True)


if __name__ == "__main__":
    main()
