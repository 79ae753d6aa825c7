"""The size classes a cluster is routed to after the scan, a model of the routing predicate, and clusters that stand
on each class's last and first size.  No GPU, no library: numpy, re and str only.

After the dedup pass a cluster has a view mode (0: every copy, 1: at most 64 distinct sequences with a sample-set
matrix and an ordinal bitmap, 2: the wide class) and the host (`build_items`, pf_api.hip) or the device
(`cluster_ninst_kernel`, pf_kernels.h, under PF_FLAG_DEVICE_PLAN) chooses key partitions, a table size and one of the
finish classes for it.  Every destination kernel has LDS arrays sized for exactly what its predicate admits, so the
predicate is restated here once (`expected_route`) from mirrored constants (`MIRROR`, held against the source text by
`source_constants`), the quantities it reads are computed from a cluster's records with dicts and str (`quantities`),
and `cases()` lists clusters built to put one quantity on one side of one term.

Generators: alleles are prefixes of one ancestor, told apart by their lengths and by single substitutions
(`prefix_alleles`); the ancestor repeats a random block where many windows are wanted from few distinct k-mers;
unrelated random alleles make every window a k-mer of its own (`random_alleles`); `mask_alleles` lands on a number of
distinct allele masks (a run of closely spaced substitution sites, each carried by a random subset of the alleles,
brings the count near the target; isolated blocks whose middle base is mutated in a subset of their own then add
exactly two masks each, and one allele cut short at its end adds exactly one); `n_allele` makes a chosen number of
slow-path rows ('N's one k apart, so that every window up to the last 'N' holds one and no run between them is a
segment).  No generator is trusted: the CPU test recomputes every case's claimed quantity with `quantities`."""
import math
import os
import re
from functools import lru_cache

import numpy as np

from kmer_content import _COMP, key_words, rand_seq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ----------------------------------------------------------------------------------------------- mirrored constants
MIRROR = {
    "FinSmall": dict(DW=1024, MR=1024, AT=256, ATL=192),
    "FinLarge": dict(DW=2048, MR=2048, AT=512, ATL=384),
    "FinLargeM": dict(DW=2048, MR=2048, AT=1024, ATL=768),
    "FinHuge": dict(DW=4096, MR=2048, AT=512, ATL=384),
    "FUSED_MAX_EXTRA": 1024, "DEDUP_EX_LDS": 1024, "DEDUP_MAX_D": 64, "DEDUP_MAX_D_WIDE": 1024, "DEDUP_MROWS": 4096,
    "DENSE_WORDS": 8192, "INSERT_SLACK": 2176, "LDS_BYTES": 163840, "MISC_WORDS": 2560,
    "AT_SLOTS": 1024, "AT_LIMIT": 768, "LT_SLOTS": 1024, "LT_LIMIT": 768, "SORT_MAX": 8192,
    "BIN_MIN_PARTS": 3, "ROOM_FACTOR": 0.9, "ONE_PART_ABOVE_D": 24.0, "SHARE_BASE": 0.99, "SHARE_MARGIN": 0.06,
    "SLOT_AT": 9600, "SMALL_TABLES": (4096, 6144),
}
# expressions the model restates: the source must still hold them, letter for letter
SOURCE_LINES = {
    "pf_kernels.h": [
        "return ((LDS_BYTES - MISC_WORDS * 4) / (8u * kw + 8u)) / 64u * 64u;",
        "uint32_t a = ns - INSERT_SLACK, b = (uint32_t)(((uint64_t)ns * 4) / 5);",
        "if (r.mode == 1 && nex <= FUSED_MAX_EXTRA && r.ninst * pc.mult < 0xFFFFFFF0ull) {",
        "one = !(L * (1.0 + pc.share * (D - 1.0)) > room) || D > 24.0;",
        "if (r.dense < FinSmall::DW * 32 - 1 && mwords <= FinSmall::MR) cls = 1;",
        "else if (r.dense < FinLarge::DW * 32 - 1 && mwords <= FinLarge::MR) cls = 2;",
        "else if (r.dense < FinHuge::DW * 32 - 1 && mwords <= FinHuge::MR) cls = 5;",
        "if (pc.NS > 4096 + INSERT_SLACK && inst <= insert_limit(4096)) { ns = 4096; nsi = 1; }",
        "else if (pc.NS > 6144 + INSERT_SLACK && inst <= insert_limit(6144)) { ns = 6144; nsi = 2; }",
        "mode1 = !sh_bad && D <= MAXD && D * Wp <= DEDUP_MROWS && worth && ((D + 31) >> 5) <= p.W;",
        "mode1 = dense_bits <= (uint64_t)DENSE_WORDS * 32;",
        "const uint64_t dense_bits = ((uint64_t)sh_total + (ex1 - ex0)) * mult;",
        "if (c + 1 > limit) { misc[1] = 1; over = true; }",
        "if (__hip_atomic_load(&at_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= CFG::ATL) break;",
        "if (__hip_atomic_load(&at_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= AT_LIMIT) break;",
        "if (__hip_atomic_load(&lt_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= LT_LIMIT) break;",
        "const bool ex_lds = ex1 - ex0 <= DEDUP_EX_LDS;",
        "const bool has_hi = p.v_nstr[c] > 32;",
    ],
    "pf_api.hip": [
        "const double room = 0.9 * (double)pf::insert_limit(NS);",
        "if (rec[ci].mode == 1 && nex <= pf::FUSED_MAX_EXTRA && NS <= 9600) {",
        "const bool fits_large = rec[ci].dense < pf::FinLarge::DW * 32 - 1 && mwords <= pf::FinLarge::MR;",
        "const bool fits_huge = rec[ci].dense < pf::FinHuge::DW * 32 - 1 && mwords <= pf::FinHuge::MR;",
        "if (rec[ci].dense < pf::FinSmall::DW * 32 - 1 && mwords <= pf::FinSmall::MR) fused = 1;",
        "} else if (fits_large) fused = 3;",
        "if (np == 1 && NS > 4096 + pf::INSERT_SLACK && inst <= pf::insert_limit(4096)) ns = 4096;",
        "else if (np == 1 && NS > 6144 + pf::INSERT_SLACK && inst <= pf::insert_limit(6144)) ns = 6144;",
        "return D > 24.0 ? 1u : (uint32_t)std::min<double>(std::ceil(est / room), (double)std::min(64u, std::max(1u, c->max_items / 2)));",
        "share = 1.0 - std::pow(0.99, (double)c->o.klength) + 0.06;",
        "const uint32_t nex_items = fused ? 0 : (nex + lim_full - 1) / lim_full;",
        "const uint32_t mwords = rec[ci].vnstr * ((W + 3) & ~3u);",
    ],
}


def _read(name):
    with open(os.path.join(REPO, "panfeed_amd", "csrc", name)) as f:
        return f.read()


def source_constants():
    """the mirrored numbers as the source states them today, and the restated expressions it no longer holds"""
    kh, api = _read("pf_kernels.h"), _read("pf_api.hip")

    def num(text, name):
        m = re.search(r"constexpr\s+uint32_t\s+(?:[A-Z_]+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
        assert m, f"{name} not found"
        return m.group(1).strip()

    out = {}
    for cfg in ("FinSmall", "FinLarge", "FinLargeM", "FinHuge"):
        m = re.search(r"struct " + cfg + r" \{ static constexpr uint32_t THREADS = \d+, DW = (\d+), MR = (\d+), AT = (\d+), "
                      r"ATL = (\d+);", kh)
        assert m, f"{cfg} not found"
        out[cfg] = dict(zip(("DW", "MR", "AT", "ATL"), map(int, m.groups())))
    for name in ("FUSED_MAX_EXTRA", "DEDUP_EX_LDS", "DEDUP_MAX_D", "DEDUP_MAX_D_WIDE", "DEDUP_MROWS", "DENSE_WORDS",
                 "INSERT_SLACK", "LDS_BYTES", "MISC_WORDS", "AT_SLOTS", "AT_LIMIT", "LT_SLOTS", "SORT_MAX"):
        out[name] = int(num(kh, name))
    lt = num(kh, "LT_LIMIT")
    assert lt == "LT_SLOTS / 4 * 3", lt
    out["LT_LIMIT"] = out["LT_SLOTS"] // 4 * 3
    out["BIN_MIN_PARTS"] = int(num(api, "BIN_MIN_PARTS"))
    m = re.search(r"const double room = ([0-9.]+) \* \(double\)pf::insert_limit\(NS\);", api)
    out["ROOM_FACTOR"] = float(m.group(1))
    m = re.search(r"return D > ([0-9.]+) \? 1u :", api)
    out["ONE_PART_ABOVE_D"] = float(m.group(1))
    m = re.search(r"share = 1\.0 - std::pow\(([0-9.]+), \(double\)c->o\.klength\) \+ ([0-9.]+);", api)
    out["SHARE_BASE"], out["SHARE_MARGIN"] = float(m.group(1)), float(m.group(2))
    m = re.search(r"__shared__ tag_t slot_at\[MULTI \? 1 : (\d+)\];", kh)
    out["SLOT_AT"] = int(m.group(1))
    out["SMALL_TABLES"] = tuple(int(x) for x in re.findall(r"if \(np == 1 && NS > (\d+) \+ pf::INSERT_SLACK", api))
    gone = [f"{name}: {ln}" for name, text in (("pf_kernels.h", kh), ("pf_api.hip", api)) for ln in SOURCE_LINES[name]
            if ln not in text]
    return out, gone


M = MIRROR


def nslots_max(kw):
    return ((M["LDS_BYTES"] - M["MISC_WORDS"] * 4) // (8 * kw + 8)) // 64 * 64


def insert_limit(ns):
    return min(ns - M["INSERT_SLACK"], ns * 4 // 5)


def ceil4(w):
    return (w + 3) & ~3


# ----------------------------------------------------------------------------------------------- quantities
_BAD = re.compile(r"[^ACGT]")
_RUN = re.compile(r"[ACGT]+")
_COMP_STR = str.maketrans("ACGTN", "TGCAN")


class Quantities:
    """what the predicates read of a cluster.  D: distinct segments (maximal A/C/G/T runs of at least k bases, by
    content, in the order the reference meets them); vinst: their windows; nex: distinct window strings that hold a
    non-ACGT letter; dense = mult (vinst + nex); inst = mult vinst; mwords = D ceil4(W); unique: distinct keys of the
    view; masks: distinct sets of distinct sequences over the keys; patterns: distinct sample sets over the keys;
    first_ords: the dense ordinal of every key's first window (clusters without slow-path rows only)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def quantities(record, k, canon, W):
    gs = record[0]
    mult = 1 if canon else 2
    col = {x: i for i, x in enumerate(sorted(gs.keys()))}
    distinct, samples, extras = {}, [], set()
    for strain in gs.keys():
        for s in gs[strain]:
            seq, comp = s.sequence, s.compsequence
            for m in _RUN.finditer(seq):
                if m.end() - m.start() >= k:
                    d = distinct.setdefault(m.group(), len(distinct))
                    if d == len(samples):
                        samples.append(set())
                    samples[d].add(col[strain])
            for m in _BAD.finditer(seq):
                p = m.start()
                for pos in range(max(0, p - k + 1), min(p, len(seq) - k) + 1):
                    spec, rev = seq[pos:pos + k], comp[pos:pos + k][::-1]
                    if canon:
                        extras.add(spec if spec <= rev else rev)
                    else:
                        extras.update((spec, rev))
    keys, first = {}, {}
    base = 0
    for seg, d in distinct.items():                          # (insertion order: the order of the representatives)
        rcs = seg.translate(_COMP_STR)[::-1]
        n = len(seg) - k + 1
        bit = 1 << d
        for pos in range(n):
            spec = seg[pos:pos + k]
            rev = rcs[len(seg) - pos - k:len(seg) - pos]
            if canon:
                key = spec if spec <= rev else rev
                keys[key] = keys.get(key, 0) | bit
                first.setdefault(key, base + pos)
            else:
                keys[spec] = keys.get(spec, 0) | bit
                keys[rev] = keys.get(rev, 0) | bit
                first.setdefault(spec, 2 * (base + pos))
                first.setdefault(rev, 2 * (base + pos) + 1)
        base += n
    D = len(distinct)
    masks = set(keys.values())
    rows = set()
    for mk in masks:
        row = set()
        for d in range(D):
            if mk >> d & 1:
                row |= samples[d]
        rows.add(frozenset(row))
    return Quantities(D=D, vinst=base, nex=len(extras), mult=mult, dense=mult * (base + len(extras)), inst=mult * base,
                      mwords=D * ceil4(W), unique=len(keys), masks=len(masks), patterns=len(rows), W=W,
                      first_ords=sorted(first.values()) if not extras else None)


# ----------------------------------------------------------------------------------------------- the route
GENERAL, SMALL, LARGE, LARGE_MULTI, HUGE = 0, 1, 2, 3, 5


class Route:
    """cls: the finish class; mode: the view; nparts / nslots: key partitions and table slots of the first attempt;
    binned: bin_kernel sorts the windows by partition first; nex_items: slow-path items beside the partitions;
    overflows: the first attempt's table runs past its limit (one partition only: how a cluster's keys fall over several
    partitions is the key hash's business); planned: plan_kernel lays the cluster out under PF_FLAG_DEVICE_PLAN"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def key(self):
        return (self.cls, self.mode, self.nparts, self.nslots)


def expected_route(q, k):
    """The predicate, once.  A fresh context has learned no line (fit.ready is false): the key-partition estimate is
    L (1 + share (D - 1)) against 0.9 of the full table's limit, and past 24 distinct sequences a cluster starts as one
    item whatever the estimate says."""
    KW = key_words(k)
    NS = nslots_max(KW)
    lim = insert_limit(NS)
    W, D = q.W, q.D
    # the view (cluster_dedup_kernel): the small class, else the wide class, else every copy
    if D <= M["DEDUP_MAX_D"] and D * ceil4(W) <= M["DEDUP_MROWS"] and (D + 31) // 32 <= W and q.dense <= M["DENSE_WORDS"] * 32:
        mode = 1
    elif D <= M["DEDUP_MAX_D_WIDE"] and (D + 31) // 32 <= W and q.dense < 0xFFFFFFF0:
        mode = 2
    else:
        mode = 0
    # key partitions of the first attempt (first_nparts)
    nparts = 1
    if mode and D:
        L = q.inst / D
        share = 1.0 - M["SHARE_BASE"] ** k + M["SHARE_MARGIN"]
        est, room = L * (1.0 + share * (D - 1.0)), M["ROOM_FACTOR"] * lim
        if est > room and not D > M["ONE_PART_ABOVE_D"]:
            nparts = int(min(math.ceil(est / room), 64))
    # the finish class (build_items / cluster_ninst_kernel)
    cls = GENERAL
    if mode == 1 and q.nex <= M["FUSED_MAX_EXTRA"] and NS <= M["SLOT_AT"]:
        def fits(cfg):
            return q.dense < M[cfg]["DW"] * 32 - 1 and q.mwords <= M[cfg]["MR"]
        if nparts == 1:
            cls = SMALL if fits("FinSmall") else LARGE if fits("FinLarge") else HUGE if fits("FinHuge") else GENERAL
        elif fits("FinLarge"):
            cls = LARGE_MULTI
    nslots = NS
    for small in M["SMALL_TABLES"]:
        if nparts == 1 and NS > small + M["INSERT_SLACK"] and q.inst <= insert_limit(small):
            nslots = small
            break
    return Route(cls=cls, mode=mode, nparts=nparts, nslots=nslots, binned=nparts >= M["BIN_MIN_PARTS"] and KW <= 2 and mode != 0,
                 nex_items=0 if cls else -(-q.nex // lim), overflows=nparts == 1 and q.unique > insert_limit(nslots),
                 planned=cls != GENERAL and nparts == 1)


# ----------------------------------------------------------------------------------------------- generators
def names_of(S):
    return [f"z{i:04d}" for i in range(S)]


def record(idx, names, alleles):
    """sample i carries alleles[i mod D]; strands alternate"""
    from panfeed_amd.classes import Seqinfo
    assert len(names) >= len(alleles), (len(names), len(alleles))
    gs, presab = {}, np.ones(len(names), dtype=np.int64)
    for i, nm in enumerate(names):
        sq = alleles[i % len(alleles)]
        gs[nm] = [Seqinfo(sq.decode(), sq.translate(_COMP).decode(), f"{nm}_{idx}", f"{nm}_c", 50 + i, 50 + i + len(sq) - 1,
                          1 if i % 2 else -1, 0)]
    return gs, idx, presab


def split(total, D, step=0):
    """D window counts that add up to `total`: equal shares (step = 0) or shares `step` apart, all different"""
    w = [total // D + step * (d - D // 2) for d in range(D)]
    w[0] += total - sum(w)
    assert min(w) >= 1 and sum(w) == total
    return w


def _sub(seq, p, rng):
    b = bytearray(seq)
    b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + int(rng.integers(0, 3))) & 3]
    return bytes(b)


def ancestor(rng, n, period=0):
    if not period:
        return rand_seq(rng, n)
    return (rand_seq(rng, period) * (n // period + 2))[:n]


def prefix_alleles(rng, k, windows, subs, period=0):
    """allele d = the first windows[d] + k - 1 bases of the ancestor with base subs[d] substituted (None: none)"""
    anc = ancestor(rng, max(windows) + k - 1, period)
    out = []
    for w, p in zip(windows, subs):
        a = anc[:w + k - 1]
        out.append(a if p is None else _sub(a, p, rng))
    assert len(set(out)) == len(out), "alleles are not distinct"
    return out


def spread_subs(k, windows):
    """a substitution per allele, each at a base of its own, k clear of either end where the allele is long enough"""
    out = []
    for d, w in enumerate(windows):
        n = w + k - 1
        out.append((k + 37 * d) % max(n - 2 * k, 1) + (k if n > 2 * k else 0))
    return out


def random_alleles(rng, k, windows):
    return [rand_seq(rng, w + k - 1) for w in windows]


def n_allele(rng, k, nex, tail):
    """a sequence whose first `nex` windows each hold an 'N' (at base f, then one every k bases: no run between them
    reaches k bases), followed by `tail` A/C/G/T bases, one segment"""
    f, j = (nex - 1) % k, (nex - 1) // k
    assert tail >= k and f + 1 + j * k == nex
    b = bytearray(rand_seq(rng, f + j * k + 1 + tail))
    for i in range(j + 1):
        b[f + i * k] = ord("N")
    return bytes(b)


def _mask_count(alleles, k):
    keys = {}
    for d, a in enumerate(alleles):
        s = a.decode()
        r = a.translate(_COMP)[::-1].decode()
        n = len(s)
        for pos in range(n - k + 1):
            spec, rev = s[pos:pos + k], r[n - pos - k:n - pos]
            key = spec if spec <= rev else rev
            keys[key] = keys.get(key, 0) | (1 << d)
    return len(set(keys.values())), len(keys)


def mask_alleles(rng, k, D, target, nwin, gap=6):
    """D alleles of at most `nwin` windows with exactly `target` distinct allele masks (canonical k-mers): see the
    module text.  Layout: k clear bases, the close sites `gap` apart, k clear bases, the isolated blocks of k + 1 bases
    (their middle base the site), clear bases up to `nwin` windows, of which one allele loses its last two when the count
    is odd."""
    n = nwin + k - 1
    anc = rand_seq(rng, n)
    alts = [b"ACGT"[(b"ACGT".index(anc[p]) + 1 + int(rng.integers(0, 3))) & 3] for p in range(n)]
    subsets = [rng.permutation(D)[:int(rng.integers(2, D - 1))] for _ in range(n)]

    def build(nclose, nblocks, cut):
        sites = [k + gap * i for i in range(nclose)]
        b0 = k + gap * nclose + k
        sites += [b0 + (k + 1) * j + k // 2 for j in range(nblocks)]
        assert b0 + (k + 1) * nblocks + 2 * k <= n, f"{target} masks do not fit {nwin} windows"
        out = [bytearray(anc) for _ in range(D)]
        for p in sites:
            for d in subsets[p]:
                out[int(d)][p] = alts[p]
        out = [bytes(a) for a in out]
        if cut:
            out[D - 1] = out[D - 1][:-2]
        return out

    lo, hi = 0, (n - 5 * k) // gap                         # the most close sites with at most target - 1 masks
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _mask_count(build(mid, 0, False), k)[0] <= target - 1:
            lo = mid
        else:
            hi = mid - 1
    for nclose in range(lo, -1, -1):                       # (the count is not quite monotone in the sites: step back if needed)
        have = _mask_count(build(nclose, 0, False), k)[0]
        if have <= target:
            break
    need = target - have
    out = build(nclose, need // 2, need % 2 == 1)
    assert len(set(out)) == D, "alleles are not distinct"
    return out


# ----------------------------------------------------------------------------------------------- cases
class Kind:
    """the engine options a case runs under; cases of a kind can share a batch"""

    def __init__(self, name, k, canon, S, max_strains):
        self.name, self.k, self.canon, self.S, self.max_strains = name, k, canon, S, max_strains
        self.W = (max_strains + 31) // 32
        self.names = names_of(S)

    def opts(self):
        return dict(klength=self.k, canon=self.canon, maf=0.0, stroi={self.names[0]})


KINDS = {kd.name: kd for kd in (
    Kind("k31", 31, True, 64, 64), Kind("k15", 15, True, 64, 64), Kind("k31_both_strands", 31, False, 64, 64),
    Kind("w16", 31, True, 64, 512), Kind("w17", 31, True, 64, 544), Kind("w24", 31, True, 64, 768), Kind("w32", 31, True, 64, 1024),
    Kind("w36", 31, True, 64, 1152),
    Kind("k63", 63, True, 32, 32), Kind("k94", 94, True, 32, 32), Kind("k126", 126, True, 32, 32))}


class Case:
    """name; kind; edges: the terms of the predicate (EDGES) whose side this cluster stands on; claim: (quantity, value)
    that puts it there; route: (class, mode) it must take; make(rng) -> alleles"""

    def __init__(self, name, kind, edges, claim, route, make, **extra):
        self.name, self.kind, self.edges, self.claim, self.route, self.make = name, KINDS[kind], tuple(edges), claim, route, make
        self.extra = extra

    def __repr__(self):
        return self.name


@lru_cache(maxsize=None)
def _built(name):
    cs = CASES[name]
    seed = int.from_bytes(name.encode(), "little") % (1 << 32)
    alleles = cs.make(np.random.default_rng(seed))
    return record(name, cs.kind.names, alleles)


def build(case):
    """the case's record (built once; treat it as read-only)"""
    return _built(case.name)


@lru_cache(maxsize=None)
def _quant(name):
    cs = CASES[name]
    return quantities(_built(name), cs.kind.k, cs.kind.canon, cs.kind.W)


def quant(case):
    return _quant(case.name)


def _dense(total, D, period=512, step=0, subs="spread", k=31):
    """D prefix alleles of a periodic ancestor whose windows add up to `total`"""
    def make(rng):
        w = split(total, D, step)
        s = spread_subs(k, w) if subs == "spread" else subs(w)
        return prefix_alleles(rng, k, w, s, period)
    return make


def _seam_subs(at, k=31):
    """a substitution per allele; the allele that holds dense ordinal `at` has its own placed so that its k windows lie
    k // 2 below `at` and the rest from `at` on"""
    def subs(w):
        out = spread_subs(k, w)
        base = 0
        for d, n in enumerate(w):
            p = at - base + k // 2
            if k - 1 <= p <= n - 1:
                out[d] = p
                return out
            base += n
        raise AssertionError("no allele holds the seam with k windows to spare")
    return subs


def _lower_subs(below, k=31):
    """substitutions only in alleles that end below dense ordinal `below`: every later allele is a bare prefix"""
    def subs(w):
        out, base = [], 0
        for d, n in enumerate(w):
            out.append(spread_subs(k, w)[d] if base + n <= below else None)
            base += n
        return out
    return subs


def _last_base_subs(k=31):
    def subs(w):
        out = spread_subs(k, w)
        out[-1] = w[-1] + k - 2                               # the last allele's last base: its last window alone is new
        return out
    return subs


def _short(D, k=31, nwin=90):
    return lambda rng: prefix_alleles(rng, k, [nwin] * D, [k + d for d in range(D)])


def _unique(total, D, k):
    return lambda rng: random_alleles(rng, k, split(total, D))


def _with_n(nex, D=26, k=31):
    def make(rng):
        w = [200] * D
        return prefix_alleles(rng, k, w, spread_subs(k, w)) + [n_allele(rng, k, nex, 2 * k)]
    return make


def _masks(D, target, nwin, k=31, gap=6):
    return lambda rng: mask_alleles(rng, k, D, target, nwin, gap)


def _all_cases():
    F, lim = MIRROR, insert_limit
    S, L_, H = F["FinSmall"], F["FinLarge"], F["FinHuge"]
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- dense ordinals
    for cfg, tag, below, above in (("FinSmall", "small", SMALL, LARGE), ("FinLarge", "large", LARGE, HUGE),
                                   ("FinHuge", "huge", HUGE, GENERAL)):
        top = F[cfg]["DW"] * 32
        subs = _last_base_subs() if cfg == "FinHuge" else "spread"
        add(f"dense_{tag}_last", "k31", [f"dense<{cfg}:in"], ("dense", top - 2), (below, 1), _dense(top - 2, 26, subs=subs))
        add(f"dense_{tag}_first_past", "k31", [f"dense<{cfg}:out"], ("dense", top - 1), (above, 1), _dense(top - 1, 26))
    top = F["DENSE_WORDS"] * 32
    add("dense_bitmap_last", "k31", ["dense<=DENSE_WORDS:in"], ("dense", top), (GENERAL, 1), _dense(top, 64))
    add("dense_wide_first", "k31", ["dense<=DENSE_WORDS:out"], ("dense", top + 1), (GENERAL, 2), _dense(top + 1, 64))
    add("dense_small_last_both_strands", "k31_both_strands", ["dense<FinSmall:in", "mult2"], ("dense", S["DW"] * 32 - 2),
        (SMALL, 1), _dense(S["DW"] * 16 - 1, 26, period=256))
    add("dense_small_first_past_both_strands", "k31_both_strands", ["dense<FinSmall:out", "mult2"], ("dense", S["DW"] * 32),
        (LARGE, 1), _dense(S["DW"] * 16, 26, period=256))
    # ---- the FinHuge half seam (prefix counts are 16-bit per half: word 2048 is dense ordinal 65536)
    add("seam_straddled", "k31", ["seam:straddled"], ("dense", H["DW"] * 32 - 2), (HUGE, 1),
        _dense(H["DW"] * 32 - 2, 25, subs=_seam_subs(65536)))
    add("seam_upper_half_empty", "k31", ["seam:upper_empty"], ("dense", H["DW"] * 32 - 2), (HUGE, 1),
        _dense(H["DW"] * 32 - 2, 26, step=2, subs=_lower_subs(65536 - 64)))
    # ---- sample-set words
    for kind, mw, cls in (("w16", S["MR"], SMALL), ("w17", S["MR"] + 256, LARGE), ("w32", L_["MR"], LARGE),
                          ("w36", L_["MR"] + 256, GENERAL)):
        side = "in" if mw in (S["MR"], L_["MR"]) else "out"
        cfg = "FinSmall" if mw <= S["MR"] + 256 else "FinLarge"
        add(f"mwords_{mw}", kind, [f"mwords<={cfg}:{side}"], ("mwords", mw), (cls, 1), _short(64))
    # (D ceil4(W) takes few values: 1 032 = 43 x 24 is the first a view of at most 64 sequences can take past FinSmall::MR,
    # and 2 052 = 57 x 36 is FinLarge::MR + 4 itself)
    add("mwords_1032", "w24", ["mwords<=FinSmall:first_past"], ("mwords", S["MR"] + 8), (LARGE, 1), _short(43))
    add("mwords_2052", "w36", ["mwords<=FinLarge:first_past"], ("mwords", L_["MR"] + 4), (GENERAL, 1), _short(57))
    add("upper_mask_word_absent", "k31", ["has_hi:no"], ("D", 32), (SMALL, 1), _short(32))
    add("upper_mask_word_present", "k31", ["has_hi:yes"], ("D", 33), (SMALL, 1), _short(33))
    # ---- distinct allele masks
    for cfg, tag, D, nwin, cls in (("FinSmall", "small", 26, 1200, SMALL), ("FinLarge", "large", 26, 2000, LARGE),
                                   ("FinLargeM", "large_multi", 24, 1700, LARGE_MULTI)):
        atl = F[cfg]["ATL"]
        for d, side in ((-1, "below"), (0, "at"), (1, "past")):
            add(f"masks_{tag}_{side}", "k31", [f"masks>={cfg}::ATL:{side}"], ("masks", atl + d), (cls, 1), _masks(D, atl + d, nwin))
    # (three times the table: at k = 31 that many masks bring more distinct k-mers than one table holds; sites three bases
    # apart under 15-base windows bring a mask with every third k-mer)
    add("masks_small_far_past", "k15", ["masks>=FinSmall::ATL:far"], ("masks", 3 * S["ATL"]), (SMALL, 1),
        _masks(26, 3 * S["ATL"], 1200, k=15, gap=3))
    for d, side in ((-1, "below"), (0, "at"), (1, "past")):
        add(f"masks_general_{side}", "w36", [f"masks>=AT_LIMIT:{side}", f"patterns>=LT_LIMIT:{side}"], ("masks", F["AT_LIMIT"] + d),
            (GENERAL, 1), _masks(64, F["AT_LIMIT"] + d, 1500), patterns=F["LT_LIMIT"] + d)
    # ---- table size and fill
    for kind, k in (("k31", 31), ("k63", 63)):
        NS = nslots_max(key_words(k))
        t1 = 6144 if NS > 6144 + F["INSERT_SLACK"] else NS
        add(f"inst_4096_last_{kind}", kind, ["inst<=limit(4096):in"], ("inst", lim(4096)), (SMALL, 1), _unique(lim(4096), 4, k), nslots=4096)
        add(f"inst_4096_first_past_{kind}", kind, ["inst<=limit(4096):out"], ("inst", lim(4096) + 1), (SMALL, 1),
            _unique(lim(4096) + 1, 4, k), nslots=t1)
        add(f"inst_6144_last_{kind}", kind, ["inst<=limit(6144):in" if t1 == 6144 else "no_6144_table"], ("inst", lim(6144)),
            (SMALL, 1), _unique(lim(6144), 4, k), nslots=t1)
    add("inst_6144_first_past_k31", "k31", ["inst<=limit(6144):out"], ("inst", lim(6144) + 1), (SMALL, 1),
        _unique(lim(6144) + 1, 4, 31), nslots=nslots_max(1))
    for kind, k in (("k31", 31), ("k63", 63), ("k94", 94), ("k126", 126)):
        full = lim(nslots_max(key_words(k)))
        for d, side in ((-1, "below"), (0, "at"), (1, "past")):
            add(f"unique_{side}_limit_{kind}", kind, [f"unique>limit(NS):{side}:KW{key_words(k)}"], ("unique", full + d), (SMALL, 1),
                _unique(full + d, 26, k), nslots=nslots_max(key_words(k)))
    # ---- slow-path rows
    fx, full = F["FUSED_MAX_EXTRA"], lim(nslots_max(1))
    add("nex_fused_last", "k31", ["nex<=FUSED_MAX_EXTRA:in"], ("nex", fx), (SMALL, 1), _with_n(fx))
    add("nex_fused_first_past", "k31", ["nex<=FUSED_MAX_EXTRA:out"], ("nex", fx + 1), (GENERAL, 1), _with_n(fx + 1))
    add("nex_one_item_last", "k31", ["nex_items:1"], ("nex", full), (GENERAL, 1), _with_n(full))
    add("nex_two_items_first", "k31", ["nex_items:2"], ("nex", full + 1), (GENERAL, 1), _with_n(full + 1))
    # ---- several partitions by the estimate (at most 24 alleles)
    add("two_partitions", "k31", ["nparts:2"], ("D", 24), (LARGE_MULTI, 1), _dense(24 * 1000, 24, period=0), nparts=2)
    add("three_partitions_binned", "k31", ["nparts:BIN_MIN_PARTS"], ("D", 24), (LARGE_MULTI, 1), _dense(24 * 1700, 24, period=0),
        nparts=3)
    add("partitions_past_the_large_class", "k31", ["nparts>1:general"], ("dense", 24 * 2800), (GENERAL, 1),
        _dense(24 * 2800, 24, period=0), nparts=4)
    return out


CASES = {cs.name: cs for cs in _all_cases()}

# every term of the predicate, both sides; the CPU test asserts that the cases' claims cover this list
EDGES = ([f"dense<{cfg}:{side}" for cfg in ("FinSmall", "FinLarge", "FinHuge") for side in ("in", "out")] +
         ["dense<=DENSE_WORDS:in", "dense<=DENSE_WORDS:out", "mult2", "seam:straddled", "seam:upper_empty"] +
         [f"mwords<={cfg}:{side}" for cfg in ("FinSmall", "FinLarge") for side in ("in", "first_past", "out")] + ["has_hi:no", "has_hi:yes"] +
         [f"masks>={t}:{side}" for t in ("FinSmall::ATL", "FinLarge::ATL", "FinLargeM::ATL", "AT_LIMIT") for side in ("below", "at", "past")] +
         ["masks>=FinSmall::ATL:far"] + [f"patterns>=LT_LIMIT:{side}" for side in ("below", "at", "past")] +
         [f"inst<=limit({t}):{side}" for t in (4096, 6144) for side in ("in", "out")] + ["no_6144_table"] +
         [f"unique>limit(NS):{side}:KW{kw}" for kw in (1, 2, 3, 4) for side in ("below", "at", "past")] +
         ["nex<=FUSED_MAX_EXTRA:in", "nex<=FUSED_MAX_EXTRA:out", "nex_items:1", "nex_items:2"] +
         ["nparts:2", "nparts:BIN_MIN_PARTS", "nparts>1:general"])


def cases(kind=None):
    return [cs for cs in CASES.values() if kind is None or cs.kind.name == kind]
