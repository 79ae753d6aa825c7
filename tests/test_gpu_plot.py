"""panfeed-plot (panfeed_amd/plot.py) against what the reference's own `plot.main()` hands to matplotlib
(tests/golden/plot.json.gz, made by tools/gen_golden_plot.py): every imshow array and alpha array to the bit, NaN at the
same places, and the lines, ticks, titles, labels, letters and file names.  The grids are built on the GPU
(pf_plotgrid_*, csrc/pf_rowfilter.hip)."""
import base64
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "plot.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
RUNS = [(f["name"], i) for f in FIX for i, r in enumerate(f["runs"]) if r["rc"] == 0]


def _arr(d):
    return np.frombuffer(base64.b64decode(d["f64"]), dtype="<f8").reshape(d["shape"])


def _bits_equal(got, exp):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got.view(np.uint64)[ok], np.ascontiguousarray(exp).view(np.uint64)[ok])


def _write(tmp_path, fx, gz=False):
    pk = tmp_path / ("kmers.tsv" + (".gz" if gz else ""))
    if gz:
        from panfeed_amd.output import ParallelGzipWriter
        w = ParallelGzipWriter(str(pk), chunk_bytes=4096)            # several members
        w.write(fx["kmers"])
        w.close()
    else:
        pk.write_text(fx["kmers"])
    pp = tmp_path / "pheno.tsv"
    pp.write_text(fx["phenotype"])
    return str(pk), str(pp)


def _kwargs(args):
    from panfeed_amd.plot import get_options
    a = get_options(["-k", "x", "-p", "y"] + args)
    return dict(column=a.column, threshold=a.threshold, start=a.start, stop=a.stop, phenotype_column=a.phenotype_column,
                sample=a.sample, minimum_pvalue=a.minimum_pvalue, nucleotides=a.nucleotides, alpha=a.alpha,
                xticks=a.xticks)


def _compare(figs, run):
    saved = [s for s in run["saved"] if s["file"] != "sequence_legend.png"]
    assert len(saved) == 3 * len(figs)
    for k, fig in enumerate(figs):
        sig, seq, hyb = saved[3 * k: 3 * k + 3]
        assert sig["file"] == f"significance_{fig.cluster}.png"
        assert seq["file"] == f"sequence_{fig.cluster}.png"
        assert hyb["file"] == f"hybrid_{fig.cluster}.png"
        _bits_equal(fig.significance, _arr(sig["figure"]["images"][0]["array"]))
        _bits_equal(fig.nucleotides, _arr(seq["figure"]["images"][0]["array"]))
        _bits_equal(fig.nucleotides, _arr(hyb["figure"]["images"][0]["array"]))
        assert sig["figure"]["images"][0]["alpha"] == 1 and seq["figure"]["images"][0]["alpha"] == 1
        _bits_equal(fig.alpha, _arr(hyb["figure"]["images"][0]["alpha"]))
        for s, title in zip((sig, seq, hyb), fig.titles):
            f = s["figure"]
            assert f["title"] == title
            assert f["ylabel"] == fig.ylabel
            assert f["hlines"] == ([] if fig.hline is None else [fig.hline])
            assert f["vlines"] == ([] if fig.vline is None else [fig.vline])
            assert f["xticks"] == fig.xticks and f["xticklabels"] == fig.xticklabels
            if fig.letters is None:
                assert f["texts"] == []
            else:
                exp = [[x, y, None if isinstance(v, float) else v]
                       for x in range(fig.letters.shape[1]) for y in range(fig.letters.shape[0])
                       for v in [fig.letters[y, x]]]
                assert f["texts"] == exp


def _figures(pk, pp, args, **kw):
    from panfeed_amd.plot import cluster_figures
    return list(cluster_figures(pk, pp, **_kwargs(args), **kw))


@pytest.mark.parametrize("name,i", RUNS, ids=[f"{n}-{i}" for n, i in RUNS])
def test_cluster_figures_equal_reference(tmp_path, name, i):
    fx = next(f for f in FIX if f["name"] == name)
    run = fx["runs"][i]
    pk, pp = _write(tmp_path, fx)
    _compare(_figures(pk, pp, run["args"]), run)


@pytest.mark.parametrize("name,i", [r for r in RUNS if r[0] == "synthetic"][:4] + [r for r in RUNS if r[0] != "synthetic"][:2])
def test_gzip_and_small_blocks_give_the_same_grids(tmp_path, name, i):
    fx = next(f for f in FIX if f["name"] == name)
    run = fx["runs"][i]
    pk, pp = _write(tmp_path, fx, gz=True)
    for block in (4096, 4096 + 37, 1 << 20):
        _compare(_figures(pk, pp, run["args"], block_bytes=block, grid_budget=64 << 10), run)


@pytest.mark.parametrize("args", [[], ["--start", "-5", "--stop", "8", "--nucleotides"], ["--start", "30", "--stop", "40", "--xticks", "5"]])
def test_command_writes_the_reference_files(tmp_path, args):
    from PIL import Image

    from panfeed_amd.plot import plot
    fx = next(f for f in FIX if f["name"] == "synthetic")
    run = next(r for r in fx["runs"] if r["args"] == args)
    pk, pp = _write(tmp_path, fx)
    out = tmp_path / "out"
    out.mkdir()
    assert plot(["-k", pk, "-p", pp, "--output-directory", str(out), "--dpi", "20"] + args) == 0
    assert sorted(os.listdir(out)) == sorted(s["file"] for s in run["saved"])
    for f in os.listdir(out):
        with Image.open(out / f) as im:
            im.verify()


def _seeded_table(path, n_rows, n_clusters, n_strains, seed):
    import pandas as pd
    rng = np.random.default_rng(seed)
    cl = rng.integers(0, n_clusters, n_rows)
    st = rng.integers(0, n_strains + 5, n_rows)                    # five strains are not phenotype strains
    pos = rng.integers(-12, 25, n_rows) + (cl % 7) * 3
    pv_choices = np.array(["1e-3", "2.5E-08", "0.5", "", "0", "1", "3.3e-05", "7e-12"] +
                          [f"{x:.3e}" for x in 10 ** rng.uniform(-9, 0, 200)])
    pv = pv_choices[rng.integers(0, len(pv_choices), n_rows)]
    kmer = np.array(["ACGT", "cGTA", "NNAC", "TTga", "GAtc"])[rng.integers(0, 5, n_rows)]
    strand = np.where(rng.random(n_rows) < 0.5, -1, 1)
    df = pd.DataFrame({"cluster": np.char.add("g", cl.astype(str)), "k-mer": kmer, "lrt-pvalue": pv,
                       "strain": np.char.add("s", st.astype(str)), "gene_start": pos, "strand": strand})
    df.to_csv(path, sep="\t", index=False)


def _grid_cells(gb, ids):
    """(cluster, strain id, position, key, count) of every non-empty cell of the clusters' grids"""
    out = []
    for c, (key, cnt) in zip(ids, gb.grids(ids)):
        s, x = np.nonzero(cnt)
        out.append((np.full(len(s), c), s, x + int(gb.min[c]), key[s, x], (cnt[s, x] >> np.uint64(32)).astype(np.int64)))
    return [np.concatenate(a) for a in zip(*out)]


def test_seeded_millions_of_rows_equal_pandas(tmp_path):
    import pandas as pd

    from panfeed_amd.plot import GridBuilder, _floats, significance_of
    path = str(tmp_path / "big.tsv")
    n_strains = 40
    _seeded_table(path, 3_000_000, 6000, n_strains, 5)
    strains = [f"s{i}" for i in range(n_strains)]
    gb = GridBuilder(strains, [0, 3, 4, 1, 5, 2])
    try:
        gb.scan_file(path, block_bytes=8 << 20)
        gb.finish()
        gb.set_significance(significance_of(gb.pvalue_texts))
        assert len(gb.clusters) >= 5000
        ids = list(range(len(gb.clusters)))
        got = [np.concatenate(x) for x in zip(*[_grid_cells(gb, ids[i:i + 700]) for i in range(0, len(ids), 700)])]
        again = [np.concatenate(x) for x in zip(*[_grid_cells(gb, ids[i:i + 700]) for i in range(0, len(ids), 700)])]
        for a, b in zip(got, again):                                   # bitwise reproducible
            assert np.array_equal(a, b)
        names = np.array(gb.clusters)
    finally:
        gb.close()
    # the reference's semantics restated with vectorised pandas: groupby max (NaN-skipping) and size
    k = pd.read_csv(path, sep="\t")
    k = k[k["strain"].isin(set(strains))]
    k["significance"] = -np.log10(k["lrt-pvalue"])
    grp = k.groupby(["cluster", "strain", "gene_start"])
    exp = pd.DataFrame({"max": grp["significance"].max(), "size": grp.size()}).reset_index()
    g = pd.DataFrame({"cluster": names[got[0]], "strain": [strains[i] for i in got[1]], "gene_start": got[2],
                      "max": _floats(got[3]), "size": got[4]})
    g = g.sort_values(["cluster", "strain", "gene_start"]).reset_index(drop=True)
    exp = exp.sort_values(["cluster", "strain", "gene_start"]).reset_index(drop=True)
    assert len(g) == len(exp)
    assert (g["cluster"].values == exp["cluster"].values).all()
    assert (g["strain"].values == exp["strain"].values).all()
    assert (g["gene_start"].values == exp["gene_start"].values).all()
    assert (g["size"].values == exp["size"].values).all()
    _bits_equal(g["max"].values, exp["max"].values.astype(np.float64))


def test_one_cluster_of_8192_strains_by_20000_positions(tmp_path):
    from panfeed_amd.plot import GridBuilder, significance_of
    rng = np.random.default_rng(3)
    n = 400_000
    st = rng.integers(0, 8192, n)
    pos = rng.integers(0, 20000, n)
    pos[0], pos[1] = 0, 19999
    lines = ["cluster\tk-mer\tlrt-pvalue\tstrain\tgene_start\tstrand"]
    lines += [f"big\tACGT\t1e-{(i % 9) + 1}\ts{s}\t{p}\t1" for i, (s, p) in enumerate(zip(st.tolist(), pos.tolist()))]
    path = tmp_path / "wide.tsv"
    path.write_text("\n".join(lines) + "\n")
    gb = GridBuilder([f"s{i}" for i in range(8192)], [0, 3, 4, 1, 5, 2])
    try:
        gb.scan_file(str(path))
        gb.finish()
        gb.set_significance(significance_of(gb.pvalue_texts))
        assert gb.clusters == ["big"] and gb.width(0) == 20000
        (key, cnt), = gb.grids([0])
        assert key.shape == (8192, 20000)
        count = (cnt >> np.uint64(32)).astype(np.int64)
        assert int(count.sum()) == n
        exp = np.zeros((8192, 20000), np.int64)
        np.add.at(exp, (st, pos), 1)
        assert np.array_equal(count, exp)
    finally:
        gb.close()


def test_scan_out_of_memory_fails_cleanly(tmp_path):
    """pf_debug_limit_alloc below the scan's record buffer (65 536 records at least): the scan fails as out of memory,
    the grid builder still closes, and with the limit lifted a fresh one gives the reference's arrays again"""
    from panfeed_amd import _lib
    from panfeed_amd.plot import GridBuilder, table_columns
    name, i = RUNS[0]
    fx = next(f for f in FIX if f["name"] == name)
    run = fx["runs"][i]
    pk, pp = _write(tmp_path, fx)
    L = _lib.load()
    gb = GridBuilder(["x"], table_columns(pk, _kwargs(run["args"])["column"]))
    try:
        _lib.check(L.pf_debug_limit_alloc(256 << 10, None))
        with pytest.raises(_lib.PanfeedHipError) as ei:
            gb.scan_file(pk)
        assert ei.value.status == _lib.ERR_OOM
        gb.close()
    finally:
        _lib.check(L.pf_debug_limit_alloc(0, None))
    _compare(_figures(pk, pp, run["args"]), run)
