#!/usr/bin/env python3
"""Generate tests/golden/plot.json.gz: what the REFERENCE's `panfeed-plot` (/root/reference/panfeed/plot.py, SURVEY 8f
row N5) hands to matplotlib, run in this container on

  * the panfeed-get-kmers outputs stored in tests/golden/n4.json.gz (the reference's own), with phenotypes made here;
  * synthetic annotated tables made here (paralogs, strand -1, lower case, NaN / empty / zero p-values, negative
    positions and gaps, strains on one side only, ties, a zoom that leaves a cluster empty, ...).

seaborn is not installed: a declared stand-in module is put in its place (as N1 declares its pyfaidx double).  It gives
`color_palette(name, n)` = the first n colours of matplotlib's `name` colormap, as RGB tuples, and a `heatmap` that does
nothing (the reference uses it only for the legend).  matplotlib runs on Agg; every Axes.imshow array and alpha array,
axhline / axvline position, xtick, title, y-label and text is captured per figure, with the saved file's name (savefig
itself writes nothing).  Only inputs made here and the reference's outputs on them are stored.

Usage: python tools/gen_golden_plot.py            (rewrites tests/golden/plot.json.gz)
"""
import base64
import gzip
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
from matplotlib.axes import Axes  # noqa: E402

SEABORN_DOUBLE = ("seaborn stand-in: color_palette(name, n) = list(matplotlib.colormaps[name].colors[:n]) as RGB "
                  "tuples; heatmap(...) draws nothing (the reference draws only the legend with it)")


def _seaborn():
    m = types.ModuleType("seaborn")
    m.color_palette = lambda name, n: [tuple(c[:3]) for c in matplotlib.colormaps[name].colors[:n]]
    m.heatmap = lambda *a, **k: None
    return m


sys.modules["seaborn"] = _seaborn()
from panfeed import plot as ref_plot  # noqa: E402  (reference)

CAPTURE = {}


def _arr(a):
    a = np.asarray(a, dtype=np.float64)
    return {"shape": list(a.shape), "f64": base64.b64encode(np.ascontiguousarray(a).astype("<f8").tobytes()).decode()}


def _fig(ax):
    """the calls on one Axes (a colour bar's Axes is its own: only the figure's first Axes is kept)"""
    return CAPTURE.setdefault(id(ax), {"images": [], "hlines": [], "vlines": [], "xticks": None, "xticklabels": None,
                                               "title": None, "ylabel": None, "texts": []})


def _install():
    orig = {n: getattr(Axes, n) for n in ("imshow", "axhline", "axvline", "set_xticks", "set_title", "set_ylabel", "text")}

    def imshow(self, X, *a, **k):
        al = k.get("alpha")
        _fig(self)["images"].append({"array": _arr(X), "dtype": str(np.asarray(X).dtype),
                                     "alpha": _arr(al) if isinstance(al, np.ndarray) else al})
        return orig["imshow"](self, X, *a, **k)

    def axhline(self, y=0, *a, **k):
        _fig(self)["hlines"].append(int(y))
        return orig["axhline"](self, y, *a, **k)

    def axvline(self, x=0, *a, **k):
        _fig(self)["vlines"].append(int(x))
        return orig["axvline"](self, x, *a, **k)

    def set_xticks(self, ticks, labels=None, **k):
        f = _fig(self)
        f["xticks"] = [int(t) for t in ticks]
        f["xticklabels"] = [int(t) for t in labels] if labels is not None else None
        return orig["set_xticks"](self, ticks, labels=labels, **k)

    def set_title(self, label, *a, **k):
        _fig(self)["title"] = label
        return orig["set_title"](self, label, *a, **k)

    def set_ylabel(self, label, *a, **k):
        _fig(self)["ylabel"] = label
        return orig["set_ylabel"](self, label, *a, **k)

    def text(self, x, y, s, *a, **k):
        _fig(self)["texts"].append([int(x), int(y), None if isinstance(s, float) and s != s else str(s)])
        return orig["text"](self, x, y, s, *a, **k)

    for n, f in (("imshow", imshow), ("axhline", axhline), ("axvline", axvline), ("set_xticks", set_xticks),
                 ("set_title", set_title), ("set_ylabel", set_ylabel), ("text", text)):
        setattr(Axes, n, f)


SAVED = []


def _savefig(fname, *a, **k):
    fig = plt.gcf()
    cap = CAPTURE.get(id(fig.axes[0])) if fig.axes else None
    CAPTURE.clear()
    SAVED.append({"file": os.path.basename(str(fname)), "figure": cap})


def run_reference(argv):
    SAVED.clear()
    CAPTURE.clear()
    old = sys.argv
    sys.argv = ["panfeed-plot"] + argv
    rc = 0
    err = None
    try:
        ref_plot.main()
    except SystemExit as e:
        rc = int(e.code or 0)
    except Exception as e:         # noqa: BLE001  (the reference's own failure, recorded)
        err = f"{type(e).__name__}: {e}"
    finally:
        sys.argv = old
        logging.getLogger("panfeed").handlers.clear()
        plt.close("all")
    return rc, err, list(SAVED)


# ---------------------------------------------------------------------------------------------------------------------
HEADER = ("cluster\tk-mer\thashed_pattern\taf\tfilter-pvalue\tlrt-pvalue\tbeta\tbeta-std-err\tintercept\tnotes\tstrain\t"
          "feature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\tgene_start\tgene_end\tstrand")


def _row(cluster, kmer, p, strain, pos, strand, fp="1.0e-02"):
    return (f"{cluster}\t{kmer}\tH\t0.1\t{fp}\t{p}\t0.5\t0.1\t0.2\t\t{strain}\tf_{strain}\tc_{strain}\t1\t{100 + pos}\t"
            f"{131 + pos}\t{pos}\t{pos + 31}\t{strand}")


def synthetic(seed):
    """an annotated table over 3 clusters x 14 strains with every corner the issue lists"""
    rng = np.random.default_rng(seed)
    strains = [f"st{i:02d}" for i in range(14)]
    pvals = ["1.00e-03", "2.50e-08", "0.5", "", "0", "1", "3.3e-05", "7e-12", "nan", "1.00e-03"]
    rows = []
    for c, (lo, hi) in (("gA", (-40, 25)), ("gB", (5, 60)), ("gC", (-10, -2))):
        for s in strains[:12]:
            for pos in range(lo, hi):
                if rng.random() < 0.25:                              # gaps
                    continue
                n = 1 + (rng.random() < 0.12) + (rng.random() < 0.05)   # paralogs
                for _ in range(n):
                    letters = "ACGTNacgtn"
                    kmer = "".join(rng.choice(list(letters), 7))
                    strand = -1 if rng.random() < 0.4 else 1
                    rows.append(_row(c, kmer, pvals[rng.integers(len(pvals))], s, pos, strand))
    # a strain of the table that is not a phenotype strain; ties in best p-value (st00/st01 share one)
    rows += [_row("gA", "ACGTACG", "1e-20", "outsider", 3, 1), _row("gA", "ACGTACG", "1e-20", "st00", 3, 1),
             _row("gA", "ACGTACG", "1e-20", "st01", 4, 1)]
    rng.shuffle(rows)
    return HEADER + "\n" + "\n".join(rows) + "\n", strains


def phenotype_text(strains, seed, extra=("nohit1", "nohit2"), drop=()):
    rng = np.random.default_rng(seed)
    names = [s for s in strains if s not in drop] + list(extra)
    lines = ["strain\tbinary\tcontinuous"]
    for s in names:
        b = int(rng.random() < 0.5)
        cont = "" if rng.random() < 0.1 else f"{rng.normal():.3f}"
        lines.append(f"{s}\t{b}\t{cont}")
    return "\n".join(lines) + "\n"


def n4_inputs():
    with gzip.open(os.path.join(REPO, "tests", "golden", "n4.json.gz"), "rb") as fh:
        fx = json.loads(fh.read().decode())["fixtures"]
    out = []
    for f in fx:
        for r in f["runs"]:
            if r["tool"] != "get_kmers" or r["rc"] != 0 or not r["stdout"]:
                continue
            if r["args"] not in (["-t", "0.01"], ["-t", "0.01", "--only-passing"]):
                continue
            out.append((f"n4:{f['case']}:{' '.join(r['args'])}", r["stdout"]))
    return out


def main():
    inputs = []
    for name, text in n4_inputs():
        strains = sorted({ln.split("\t")[10] for ln in text.split("\n")[1:] if ln and ln.split("\t")[10]})
        pheno = phenotype_text(strains, len(inputs), drop=strains[:1] if len(strains) > 1 else ())
        argsets = [[], ["--phenotype-column", "binary"], ["-t", "0.01", "--alpha", "0.2"]]
        inputs.append({"name": name, "kmers": text, "phenotype": pheno, "argsets": argsets})
    syn, strains = synthetic(7)
    pheno = phenotype_text(strains, 99, drop=strains[-1:])
    inputs.append({"name": "synthetic", "kmers": syn, "phenotype": pheno, "argsets": [
        [], ["--phenotype-column", "binary"], ["--phenotype-column", "continuous"],
        ["-t", "0.05", "--minimum-pvalue", "1e-6", "--alpha", "0.3"],
        ["--start", "-5", "--stop", "8", "--nucleotides"],
        ["--start", "-5", "--stop", "8", "--nucleotides", "--phenotype-column", "binary"],
        ["--start", "30", "--stop", "40", "--xticks", "5"],                 # gC has no row there: "Skipping"
        ["--xticks", "7", "-c", "filter-pvalue"],
        ["-c", "no-such-column"], ["--phenotype-column", "no-such-column"],
        ["--sample", "2"], ["--alpha", "-1"], ["--start", "3"], ["--start", "5", "--stop", "1"],
    ]})
    _install()
    ref_plot.plt.savefig = _savefig
    fixtures = []
    with tempfile.TemporaryDirectory() as d:
        for inp in inputs:
            pk, pp = os.path.join(d, "kmers.tsv"), os.path.join(d, "pheno.tsv")
            with open(pk, "w") as fh:
                fh.write(inp["kmers"])
            with open(pp, "w") as fh:
                fh.write(inp["phenotype"])
            runs = []
            for extra in inp["argsets"]:
                argv = ["-k", pk, "-p", pp, "--output-directory", d, "--dpi", "20", "--format", "png"] + extra
                rc, err, saved = run_reference(argv)
                if err:
                    print(f"{inp['name']} {extra}: the reference fails ({err}); not kept", file=sys.stderr)
                    continue
                runs.append({"args": extra, "rc": rc, "saved": saved})
            fixtures.append({"name": inp["name"], "kmers": inp["kmers"], "phenotype": inp["phenotype"], "runs": runs})
    import pandas as pd
    path = os.path.join(REPO, "tests", "golden", "plot.json.gz")
    meta = {"pandas": pd.__version__, "numpy": np.__version__, "matplotlib": matplotlib.__version__,
            "seaborn": SEABORN_DOUBLE}
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(json.dumps({"meta": meta, "fixtures": fixtures}).encode())
    print(path, sum(len(f["runs"]) for f in fixtures), "runs")


if __name__ == "__main__":
    main()
