"""`python -m panfeed_amd.plot`: the reference's `panfeed-plot` (/root/reference/panfeed/plot.py).

Options, defaults, refusals (their order and exit status) and output file names are the reference's (`plot.py:35-136`,
`:145-158`, `:165-167`, `:196-198`), plus `--device` as the downstream tools have.  What the reference does with one
pandas frame of the whole annotated table and three `pivot_table`s per cluster (`:195-305`) is done here by
`pf_plotgrid_*` (csrc/pf_rowfilter.hip): the table streams through the GPU in blocks of complete lines -- a `.gz` of small
members, as `panfeed-get-kmers --gz-output` writes it, goes up compressed and is inflated there -- and every
cluster's grid (largest significance, row count, the one row's letter) is built there with integer atomics.  What is
left on the host is small and goes through the reference's own pandas / numpy statements: the phenotype, the parse of
the distinct p-value texts and their -log10, the order of the strains, the hybrid normalisation.  Rendering is
matplotlib's, as the reference's (`:320-397`), without seaborn.

`cluster_figures` is the API under the command: one `ClusterFigure` per cluster, holding what is handed to matplotlib.
"""
import argparse
import ctypes as C
import io
import logging
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import __version__, _lib
from .downstream import GZ_BLOCK_DIVISOR, DeviceTable, open_table, route_file

logger = logging.getLogger("panfeed")

BLOCK_BYTES = 64 << 20            # text per pf_plotgrid_scan
GRID_BUDGET = 4 << 30             # device bytes of the grids built at one time (16 per cell)
COLUMNS = ("cluster", "strain", "gene_start", "k-mer", "strand")
BASE2INT = {"A": 0, "G": 1, "T": 2, "C": 3}        # plot.py:207-210


class Refusal(Exception):
    """an input the reference refuses with a warning and exit status 1"""


def get_options(argv=None):
    parser = argparse.ArgumentParser(prog="panfeed-plot", description="Plot association results from panfeed")
    parser.add_argument("-k", "--kmers", required=True, help="TSV file containing the output of panfeed-get-kmers")
    parser.add_argument("-c", "--column", default="lrt-pvalue",
                        help="P-value column in the associations file (default %(default)s)")
    parser.add_argument("-t", "--threshold", type=float, default=1,
                        help="Association p-value threshold (default %(default).2f)")
    parser.add_argument("-p", "--phenotype", required=True, help="Phenotype file in TSV format, used to list all strains")
    parser.add_argument("--phenotype-column", default=None,
                        help="Column in phenotype TSV file for sorting (default is sorting by p-values)")
    parser.add_argument("--sample", type=float, default=None,
                        help="Only show a randomly picked set of sample (a value between 0 and 1 indicating the "
                             "proportion to show, default all)")
    parser.add_argument("--start", type=int, default=None,
                        help="Relative position to start the plots (default all available positions)")
    parser.add_argument("--stop", type=int, default=None,
                        help="Relative position to end the plots (default all available positions)")
    parser.add_argument("--format", choices=("png", "tiff", "pdf", "svg"), default="png",
                        help="Output format for plots (default %(default)s)")
    parser.add_argument("--output-directory", default=".", help="Output directory for the plots (default %(default)s)")
    parser.add_argument("--dpi", type=int, default=300, help="Output resolution (DPI, default %(default)d)")
    parser.add_argument("--minimum-pvalue", type=float, default=1E-10,
                        help="Minimum p-value for color and transparency (default %(default).2e)")
    parser.add_argument("--nucleotides", action="store_true", default=False,
                        help="Draw nucleotide sequence on all plots "
                             "(WARNING: only makes sense if few samples and positions are considered)")
    parser.add_argument("--alpha", type=float, default=0,
                        help="Opacity for non-passing k-mers (between 0 and 1, 0 indicates full transparency, "
                             "default %(default).2f)")
    parser.add_argument("--xticks", type=int, default=200, help="Spacing for ticks on x axis (default %(default)d)")
    parser.add_argument("--height", type=float, default=9., help="Figure height (inches, default %(default).1f)")
    parser.add_argument("--width", type=float, default=10., help="Figure width (inches, default %(default).1f)")
    parser.add_argument("-v", action="count", default=0, help="Increase verbosity level")
    parser.add_argument("--version", action="version", version="%(prog)s " + __version__)
    parser.add_argument("--device", type=int, default=0, help="GPU the grids are built on")
    parser.add_argument("--host-gunzip", action="store_true", default=False,
                        help="inflate a .gz table on the host (by default a file of small members, as panfeed-get-kmers "
                             "--gz-output writes, or a bgzip'd file (BGZF) is inflated on the GPU)")
    parser.add_argument("--gpu-gunzip-large", action="store_true", default=False,
                        help="inflate any other .gz table on the GPU as well -- what gzip, pigz or --compress wrote: large members, "
                             "decoded in parallel inside a member (off by default; --host-gunzip wins over it)")
    return parser.parse_args(argv)


def check_options(args):
    """the reference's refusals, in its order (plot.py:145-158); a Refusal's message is its warning"""
    if args.sample is not None and (args.sample > 1 or args.sample < 0):
        raise Refusal("--sample should be between 0 and 1")
    if args.alpha > 1 or args.alpha < 0:
        raise Refusal("--alpha should be between 0 and 1")
    if (args.start is not None and args.stop is None) or (args.start is None and args.stop is not None):
        raise Refusal("both --start and --stop are needed")
    if args.start is not None and args.start > args.stop:
        raise Refusal("--start should be lower than --stop")
    if args.nucleotides and (args.sample is None or args.start is None):
        logger.warning("drawing nucleotide sequences without zooming in might "
                       "increase plotting time and memory consumption "
                       "while generating useless plots")


@dataclass
class Phenotype:
    index: list                   # the strains, in the phenotype's order after dropna / sort / sample
    pbinary: bool
    yindex: Optional[int]
    sort_by_phenotype: bool


def read_phenotype(path, phenotype_column=None, sample=None):
    """plot.py:162-191, the reference's statements"""
    import pandas as pd
    p = pd.read_csv(path, sep="\t", index_col=0)
    pbinary = False
    yindex = None
    if phenotype_column is not None:
        if phenotype_column not in p.columns:
            raise Refusal(f"phenotype file does not have the {phenotype_column} column")
        p = p[phenotype_column].dropna().sort_values(ascending=False)
        if sample is not None:
            p = p.sample(frac=sample)
        pvalues = set(p.values)
        if len(pvalues) == 2 and 1 in pvalues and 0 in pvalues:
            logger.info("Phenotype is binary")
            pbinary = True
            yindex = [i for i, x in enumerate(p) if i > 0 and x != p.iloc[i - 1]]
            yindex = yindex[0] if len(yindex) > 0 else None
        else:
            logger.info("Phenotype is continuos")
        logger.info(f"sorting samples by their {phenotype_column} phenotype")
        logger.info("ties will be broken by association p-value")
    else:
        logger.info("sorting samples by their lowest association p-value")
        if sample is not None:
            p = p.sample(frac=sample)
    logger.info(f"plots will include {len(set(p.index))} samples")
    return Phenotype(list(p.index), pbinary, yindex, phenotype_column is not None)


def table_columns(path, column):
    """the column indices (cluster, strain, gene_start, k-mer, strand, `column`) from the table's header line"""
    with open_table(path) as fh:
        header = fh.readline().rstrip(b"\r\n").decode().split("\t")
    if column not in header:
        raise Refusal(f"k-mer file does not have the {column} column")
    missing = [c for c in COLUMNS if c not in header]
    if missing:
        raise KeyError(f"{path}: no {', '.join(missing)} column")
    return [header.index(c) for c in COLUMNS] + [header.index(column)]


@dataclass
class ClusterFigure:
    """what the reference hands to matplotlib for one cluster (plot.py:320-397)"""
    cluster: str
    significance: np.ndarray           # g.values, float64, strains x positions
    nucleotides: np.ndarray            # b.values, float64 (0..3, 99 for paralogs, NaN)
    alpha: np.ndarray                  # the hybrid's alpha, float64
    letters: Optional[np.ndarray]      # t.values (object: a letter, '-', or NaN) with --nucleotides
    strains: list
    positions: np.ndarray              # the columns: min..max gene_start
    hline: Optional[int]               # axhline row (binary phenotype)
    vline: Optional[int]               # axvline column (gene start)
    xticks: List[int]
    xticklabels: List[int]
    titles: tuple                      # significance, sequence, hybrid
    ylabel: str
    stats: dict = field(default_factory=dict)


def _keys(sig):
    """64-bit ordered integer keys of float64 values (0 for NaN): bit operations only"""
    bits = np.ascontiguousarray(sig, dtype=np.float64).view(np.uint64)
    neg = (bits >> np.uint64(63)).astype(bool)
    keys = np.where(neg, ~bits, bits | np.uint64(1 << 63))
    keys[np.isnan(sig)] = 0
    return keys


def _floats(keys):
    """the inverse of _keys; NaN where the key is 0"""
    pos = (keys >> np.uint64(63)).astype(bool)
    bits = np.where(pos, keys & np.uint64((1 << 63) - 1), ~keys)
    out = bits.view(np.float64).copy()
    out[keys == 0] = np.nan
    return out


def significance_of(texts):
    """-log10 of the distinct p-value texts (plot.py:202): parsed as a column of pandas' read_csv, as the reference
    reads them, then the reference's own expression"""
    import pandas as pd
    body = b"i\tp\n" + b"".join(b"%d\t%s\n" % (i, t) for i, t in enumerate(texts))
    col = pd.read_csv(io.BytesIO(body), sep="\t", index_col=0)["p"]
    return np.asarray(-np.log10(col), dtype=np.float64)


_SCALAR = np.full(256, np.nan)
for _b, _v in BASE2INT.items():
    _SCALAR[ord(_b)] = _v


class GridBuilder(DeviceTable):
    """pf_plotgrid: the annotated table streamed through the device, then grids for batches of clusters"""

    entry = ("pf_plotgrid_create", "pf_plotgrid_destroy", "pf_plotgrid_members_begin", "pf_plotgrid_members_header")
    device_gunzip_files = 0         # files, over all builders, that went the device gunzip route to their end
    fallback_files = 0              # and files the automatic mode began there and read again through gzip

    def __init__(self, strains, columns, start=None, stop=None, device=0):
        super().__init__()
        names = [str(s).encode() for s in strains]
        zoom = start is not None
        arr, lens = _lib.c_strings(names)
        self.args = (int(device), arr, lens, len(names), (C.c_int32 * 6)(*columns), 1 if zoom else 0, int(start) if zoom else 0,
                     int(stop) if zoom else 0)
        self.fallbacks = 0              # files the automatic mode began on the device and read again through gzip
        self._create(*self.args)        # (and again, for an empty grid: _fell_back)
        self.n_strains = len(names)

    def _fell_back(self):
        """a file refused part-way has left rows in the grid: it starts over on an empty one"""
        self.fallbacks += 1
        self._create(*self.args)

    def scan_file(self, path, block_bytes=None, device_gunzip=None, large_members=None, piece_bytes=None):
        """The data lines of the annotated table into the grid.  A .gz made of small members with the plain gzip header is
        inflated on the device and scanned there, as device_gunzip says (downstream.route_file: None tries it for such a
        file and reads the file again through gzip when a block is not taken, True raises NotTaken then, False never
        tries); block_bytes then counts compressed bytes.  Any other file is read block by block through the host.
        large_members: True, the large-member route as well -- any .gz is tried on the device; None leaves the switch as
        DeviceTable.set_large_members set it."""
        def members():                               # True, or None when a block was not taken
            return self._members_pass(path, block_bytes or BLOCK_BYTES // GZ_BLOCK_DIVISOR, self.L.pf_plotgrid_scan_members) or None

        def host():
            self._plain_pass(path, block_bytes or BLOCK_BYTES, self.L.pf_plotgrid_scan)
            return True

        route_file(path, device_gunzip, members, host, GridBuilder, self._fell_back, large_members=self._large(large_members, piece_bytes))

    def finish(self):
        nc, npv, nr = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _lib.check(self.L.pf_plotgrid_finish(self.h, C.byref(nc), C.byref(npv), C.byref(nr)))
        nc, npv = int(nc.value), int(npv.value)
        names, off = C.c_void_p(), C.POINTER(C.c_uint64)()
        mn, mx, rows = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)()
        _lib.check(self.L.pf_plotgrid_clusters(self.h, C.byref(names), C.byref(off), C.byref(mn), C.byref(mx), C.byref(rows)))
        offs = np.ctypeslib.as_array(off, (nc + 1,)).copy() if nc else np.zeros(1, np.uint64)
        raw = C.string_at(names, int(offs[-1])) if nc else b""
        self.clusters = [raw[offs[i]:offs[i + 1]].decode() for i in range(nc)]
        self.min = np.ctypeslib.as_array(mn, (nc,)).copy() if nc else np.zeros(0, np.int32)
        self.max = np.ctypeslib.as_array(mx, (nc,)).copy() if nc else np.zeros(0, np.int32)
        self.rows = np.ctypeslib.as_array(rows, (nc,)).copy() if nc else np.zeros(0, np.uint64)
        texts, toff = C.c_void_p(), C.POINTER(C.c_uint64)()
        _lib.check(self.L.pf_plotgrid_pvalues(self.h, C.byref(texts), C.byref(toff)))
        to = np.ctypeslib.as_array(toff, (npv + 1,)).copy() if npv else np.zeros(1, np.uint64)
        raw = C.string_at(texts, int(to[-1])) if npv else b""
        self.pvalue_texts = [raw[to[i]:to[i + 1]] for i in range(npv)]
        self.n_records = int(nr.value)

    def set_significance(self, sig):
        keys = np.ascontiguousarray(_keys(sig), dtype=np.uint64)
        _lib.check(self.L.pf_plotgrid_set_significance(self.h, keys.ctypes.data if len(keys) else None))

    def width(self, i):
        return int(self.max[i]) - int(self.min[i]) + 1

    def grids(self, ids):
        """[(key grid, count | letter grid)] of clusters `ids`, each n_strains x width, uint64"""
        widths = [self.width(i) for i in ids]
        cells = sum(widths) * self.n_strains
        key = np.empty(cells, np.uint64)
        cnt = np.empty(cells, np.uint64)
        idarr = np.asarray(ids, dtype=np.uint32)
        _lib.check(self.L.pf_plotgrid_grids(self.h, idarr.ctypes.data, len(ids), key.ctypes.data, cnt.ctypes.data))
        out, o = [], 0
        for w in widths:
            n = w * self.n_strains
            out.append((key[o:o + n].reshape(self.n_strains, w), cnt[o:o + n].reshape(self.n_strains, w)))
            o += n
        return out

    def stats(self):
        b, ln, r, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        _lib.check(self.L.pf_plotgrid_stats(self.h, C.byref(b), C.byref(ln), C.byref(r), C.byref(ms)))
        gm, gt, gms, gdev = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_uint64()
        _lib.check(self.L.pf_plotgrid_gunzip_stats(self.h, C.byref(gm), C.byref(gt), C.byref(gms), C.byref(gdev)))
        return {"bytes_scanned": int(b.value), "lines": int(ln.value), "records": int(r.value),
                "device_ms": float(ms.value),
                "members_inflated": int(gm.value), "text_bytes_inflated": int(gt.value), "inflate_ms": float(gms.value),
                "inflate_device_bytes": int(gdev.value), "gunzip_fallbacks": self.fallbacks}


def _figure(gene, key, cnt, ph, names, ids_of, mn, mx, threshold, minimum_pvalue, alpha, xticks, nucleotides):
    """one cluster's arrays from its device grids, through the reference's statements (plot.py:261-375)"""
    import pandas as pd
    sig = _floats(key)
    count = (cnt >> np.uint64(32)).astype(np.int64)
    letter = (cnt & np.uint64(0xFF)).astype(np.uint8)
    one = count == 1
    if ph.sort_by_phenotype:
        ids = [ids_of[s] for s in ph.index]                             # g.loc[p.index]
    else:
        # the pivot keeps the strains with a non-NaN cell, in sorted order; the reindex adds the rest behind them,
        # sorted; then the order by best significance, by the reference's own (unstable) sort of the same Series
        has = (key != 0).any(axis=1)
        pre = sorted(n for n, h in zip(names, has) if h) + sorted(n for n, h in zip(names, has) if not h)
        pre_ids = np.asarray([ids_of[n] for n in pre], dtype=np.int64)
        s = sig[pre_ids]
        best = pd.Series(np.where(np.isnan(s), 0, s).max(axis=1), index=pd.Index(pre, dtype=object))
        order = best.sort_values(ascending=False).index
        ids = [ids_of[n] for n in order]
    ids = np.asarray(ids, dtype=np.int64)
    strains = [names[i] for i in ids]
    g = sig[ids]
    b = np.where(count[ids] >= 2, 99.0, np.where(one[ids], _SCALAR[letter[ids]], np.nan))
    t = None
    if nucleotides:
        lt = np.where(one & (letter != 0), letter, 0)
        t = np.full(count.shape, np.nan, dtype=object)
        t[count >= 2] = "-"
        sel = lt != 0
        t[sel] = np.array([chr(c) for c in range(256)], dtype=object)[lt[sel]]
        present = (count >= 2).any(axis=1) | (lt != 0).any(axis=1)       # the strains the text pivot keeps
        t[~present, :] = "-"
        t = t[ids]
    positions = np.arange(int(mn), int(mx) + 1)
    vline = int(-mn) if mn <= 0 <= mx else None
    tick = positions % xticks == 0
    # the hybrid's alpha (plot.py:371-375)
    h = pd.DataFrame(g)
    h = h.fillna(h.min().min())
    h = (h - -np.log10(threshold)) / (-np.log10(minimum_pvalue) - -np.log10(threshold))
    h[h < alpha] = alpha
    h[h > 1] = 1
    h[np.isnan(h)] = alpha
    return ClusterFigure(
        cluster=gene, significance=g, nucleotides=b, alpha=h.values, letters=t, strains=strains, positions=positions,
        hline=ph.yindex if ph.pbinary else None, vline=vline,
        xticks=[int(i) for i in np.nonzero(tick)[0]], xticklabels=[int(x) for x in positions[tick]],
        titles=(f"significant k-mers {gene}", f"nucleotide sequence {gene}", f"significant k-mers {gene}"),
        ylabel=f"{g.shape[0]} samples")


def _figures(kmers, ph, columns, threshold=1, start=None, stop=None, minimum_pvalue=1e-10, nucleotides=False,
             alpha=0, xticks=200, device=0, block_bytes=None, grid_budget=None, device_gunzip=None, large_members=False):
    strains = list(dict.fromkeys(ph.index))
    gb = GridBuilder(strains, columns, start, stop, device)
    try:
        gb.scan_file(kmers, block_bytes, device_gunzip, large_members)
        gb.finish()
        gb.set_significance(significance_of(gb.pvalue_texts))
        ids_of = {s: i for i, s in enumerate(strains)}
        logger.info(f"preparing plots for {len(gb.clusters)} gene clusters")
        order = sorted(range(len(gb.clusters)), key=lambda i: gb.clusters[i])
        budget = max(1, (grid_budget or GRID_BUDGET) // 16)
        i = 0
        while i < len(order):
            batch, cells = [], 0
            while i < len(order):
                c = order[i]
                need = gb.width(c) * len(strains) if gb.rows[c] else 0
                if batch and cells + need > budget:
                    break
                batch.append(c)
                cells += need
                i += 1
            with_rows = [c for c in batch if gb.rows[c]]
            grids = dict(zip(with_rows, gb.grids(with_rows))) if with_rows else {}
            for c in batch:
                gene = gb.clusters[c]
                logger.info(f"preparing plots for {gene}")
                if c not in grids:
                    logger.warning(f"Skipping {gene}")
                    continue
                key, cnt = grids.pop(c)
                fig = _figure(gene, key, cnt, ph, strains, ids_of, gb.min[c], gb.max[c], threshold, minimum_pvalue, alpha, xticks, nucleotides)
                fig.stats = gb.stats()
                yield fig
    finally:
        gb.close()


def cluster_figures(kmers, phenotype, column="lrt-pvalue", threshold=1, start=None, stop=None, phenotype_column=None,
                    sample=None, minimum_pvalue=1e-10, nucleotides=False, alpha=0, xticks=200, device=0,
                    block_bytes=None, grid_budget=None, device_gunzip=None, large_members=False):
    """One ClusterFigure per cluster of the annotated table `kmers` (panfeed-get-kmers' output; a .gz of small members, as
    its --gz-output writes, is inflated on the GPU, any other .gz read through gzip: device_gunzip as
    GridBuilder.scan_file's) that has rows in the zoom, in sorted() order.  `phenotype` is the phenotype TSV's path.
    Raises Refusal where the reference exits with status 1."""
    ph = read_phenotype(phenotype, phenotype_column, sample)
    columns = table_columns(kmers, column)
    yield from _figures(kmers, ph, columns, threshold, start, stop, minimum_pvalue, nucleotides, alpha, xticks, device,
                        block_bytes, grid_budget, device_gunzip, large_members)


def _colormaps():
    """plot.py:231-239; sns.color_palette('tab20', n) is the first n colours of matplotlib's tab20"""
    import matplotlib.pyplot as plt
    from matplotlib import colors
    tab20 = list(plt.get_cmap("tab20").colors)
    cmap1 = plt.get_cmap("viridis").copy()
    cmap1.set_bad("xkcd:grey")
    cmap1.set_under("xkcd:light grey")
    cmap2 = colors.LinearSegmentedColormap.from_list("nucleotides", tab20[:4], 4)
    cmap2.set_bad("xkcd:grey")
    cmap2.set_over(tab20[4])
    return cmap1, cmap2


def render(fig, args, cmap1, cmap2):
    """the three figures of one cluster (plot.py:320-397)"""
    import matplotlib.pyplot as plt
    from mpl_toolkits.axes_grid1 import make_axes_locatable
    gene = fig.cluster
    for kind in ("significance", "sequence", "hybrid"):
        f, ax = plt.subplots(figsize=(args.width, args.height))
        if kind == "significance":
            im = ax.imshow(fig.significance, cmap=cmap1, vmin=-np.log10(args.threshold),
                           vmax=-np.log10(args.minimum_pvalue), aspect="auto", interpolation="none",
                           rasterized=True, alpha=1)
        else:
            im = ax.imshow(fig.nucleotides, cmap=cmap2, vmin=0, vmax=3, aspect="auto", interpolation="none",
                           rasterized=True, alpha=1 if kind == "sequence" else fig.alpha)
        if fig.letters is not None:
            for x in range(fig.letters.shape[1]):
                for y in range(fig.letters.shape[0]):
                    ax.text(x, y, fig.letters[y, x], ha="center", va="center")
        ax.set_yticks([])
        if fig.hline is not None:
            ax.axhline(fig.hline, lw=1, color="black")
        if fig.vline is not None:
            ax.axvline(fig.vline, lw=1, color="black")
        ax.set_xticks(fig.xticks, labels=fig.xticklabels)
        ax.set_title(fig.titles[("significance", "sequence", "hybrid").index(kind)])
        ax.set_xlabel("position relative to gene start")
        ax.set_ylabel(fig.ylabel)
        if kind == "significance":
            divider = make_axes_locatable(ax)
            cax = divider.append_axes("right", size="2.5%", pad=0.05)
            coba = plt.colorbar(im, cax=cax)
            coba.set_label("-log10 p-value")
        name = f"{kind}_{gene}.{args.format}"
        plt.savefig(os.path.join(args.output_directory, name), dpi=args.dpi, bbox_inches="tight")
        logger.info(f"saved plot {name}")
        plt.close()


def render_legend(args, cmap2):
    """the nucleotide colour key (plot.py:400-414), four squares labelled A G T C, matplotlib only"""
    import matplotlib.pyplot as plt
    f, ax = plt.subplots(figsize=(3, 0.7))
    ax.imshow([[0, 1, 2, 3]], cmap=cmap2, vmin=0, vmax=3, aspect="equal")
    for x, s in enumerate("AGTC"):
        ax.text(x, 0, s, ha="center", va="center", size=16, weight="bold")
    ax.set_xticks([])
    ax.set_yticks([])
    name = f"sequence_legend.{args.format}"
    plt.savefig(os.path.join(args.output_directory, name), dpi=args.dpi, bbox_inches="tight")
    logger.info(f"Saved nucleotide color key at {name}")
    plt.close()


def _set_logging(v):
    logger.setLevel(logging.DEBUG)
    if not logger.handlers:
        ch = logging.StreamHandler()
        ch.setLevel(logging.DEBUG if v >= 1 else logging.INFO)
        ch.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(message)s", "%H:%M:%S"))
        logger.addHandler(ch)


def plot(argv=None):
    """panfeed-plot; returns the exit status"""
    args = get_options(argv)
    _set_logging(args.v)
    try:
        check_options(args)
        ph = read_phenotype(args.phenotype, args.phenotype_column, args.sample)
        columns = table_columns(args.kmers, args.column)
    except Refusal as e:
        logger.warning(str(e))
        return 1
    import matplotlib
    if "matplotlib.pyplot" not in sys.modules:
        matplotlib.use("Agg")
    cmap1, cmap2 = _colormaps()
    for fig in _figures(args.kmers, ph, columns, args.threshold, args.start, args.stop, args.minimum_pvalue,
                        args.nucleotides, args.alpha, args.xticks, args.device,
                        device_gunzip=False if args.host_gunzip else None, large_members=getattr(args, "gpu_gunzip_large", False)):
        render(fig, args, cmap1, cmap2)
    render_legend(args, cmap2)
    return 0


def main_plot():
    sys.exit(plot())


if __name__ == "__main__":
    main_plot()
