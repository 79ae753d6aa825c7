"""Inputs of the weak-hash tests and what can be said about them without a GPU.  numpy and str only.

Five places of the library are exact because a content hash is followed by a compare of the content itself (DESIGN.md
section 2, "Hash independence").  libpanfeed_hip_weakhash.so ANDs those hashes with a mask, so that different content
meets under one hash and the compares run in that role.  This file holds the clusters that reach each compare, the list
of runs (case x masked sites x mask x consider_missing) that tests/weakhash_worker.py goes through with the variant and
tests/test_gpu_weak_hash.py asserts on, and the predictions: how many clusters must fall back at mask 0, how many allele
masks a cluster's k-mers carry.
"""
import numpy as np

import kmer_content as kc

CONTROL = 0xFFFFFFFFFFFFFFFF
HIGH4 = 0xF000000000000000            # the low bits every slot is chosen by are constant, the identity bits vary
MASKS = (CONTROL, 0, 0x7, HIGH4)
WIDE_MASK = 0x7FF                     # 2 048 hash values: 70 .. 100 distinct sequences keep more than 64 of them, so the small
                                      # class hands the cluster to the wide class, where a pair meets under one value in
                                      # seven clusters of ten (all five clusters without one: 3 chances in 10 000)
# pf_debug_set_hash_mask_site's sites; None = every site (pf_debug_set_hash_mask)
SITE_DEDUP, SITE_UNIT, SITE_ROWS, SITE_TEXT = 0, 1, 2, 3
# pf_debug_weakhash_counts
COUNTERS = ("dedup_small", "dedup_wide", "unit", "rows", "rowfilter", "strain", "rows_handed_over", "rows_gave_up")
VERIFY_COUNTERS = COUNTERS[:6]        # a compare failed behind an equal hash: all 0 at the control mask

DEDUP_MIN_SEGS = 4                    # cluster_dedup_kernel: n >= 4
SMALL_MAX_D = 64                      # DEDUP_MAX_D
POOL_WORDS_SMALL = 2048               # DedupSmall::POOL, 64-bit words
UNIT_PAIRS = 2048
MASK_TABLE_CAP = 768                  # AT_LIMIT: entries of a round's mask table in rows_kernel, at most
KEY_LIMIT = 7424                      # keys of one work item

SMALL_K = (5, 31, 64, 126)


def _mut(seq, positions):
    b = bytearray(seq)
    for p in positions:
        b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1) % 4]
    return bytes(b)


def cluster(idx, names, seqs, absent=()):
    """a reference-shaped record: sample i carries sequence i mod D, strands alternate; `absent` strains have no gene"""
    from panfeed_amd.classes import Seqinfo
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    col = {x: i for i, x in enumerate(sorted(names))}
    gs, presab = {}, np.zeros(len(names), dtype=np.int64)
    carriers = [nm for nm in names if nm not in absent]
    assert len(set(seqs)) == len(seqs) <= len(carriers), (idx, len(seqs), len(carriers))
    for nm in absent:
        gs[nm] = []
    for i, nm in enumerate(carriers):
        sq = seqs[i % len(seqs)]
        gs[nm] = [Seqinfo(sq.decode(), sq.translate(comp).decode(), f"{nm}_{idx}", f"{nm}_c", 50 + i, 50 + i + len(sq) - 1,
                          1 if i % 2 else -1, 0)]
        presab[col[nm]] = 1
    return gs, idx, presab


def sequences(rec):
    """the cluster's sequences in sample order (one all-ACGT sequence per carrier: one segment each)"""
    return [s.sequence.encode() for nm in rec[0] for s in rec[0][nm]]


def n_distinct(rec):
    """distinct (content, length) pairs: a Python bytes object is both"""
    return len(set(sequences(rec)))


def eligible(rec):
    return len(sequences(rec)) >= DEDUP_MIN_SEGS


def predict_dedup(recs):
    """at mask 0 every sequence of a cluster meets the cluster's first one under one hash: (clusters whose compare must
    fail = the small-class counter, clusters that must still take the view of distinct sequences = n_dedup_clusters)"""
    el = [r for r in recs if eligible(r)]
    return sum(n_distinct(r) >= 2 for r in el), sum(n_distinct(r) == 1 for r in el)


def a_tail_family(rng, k, nwin):
    """X, X + 'A', X + 'AAAA', X + 33 'A' and X without its last base; X ends in 'A' after `nwin` windows: 'A' packs to the
    zero bits of the padding, so X, X + 'A' and X + 'AAAA' are the same words at three lengths"""
    X = kc.rand_seq(rng, nwin + k - 2) + b"CA"
    return [X, X + b"A", X + b"AAAA", X + b"A" * 33, X[:-1]]


# ------------------------------------------------------------------------------------------------- small class
def small_case(k):
    """the batch of one k for cluster_dedup_kernel<DedupSmall>: at most 64 distinct sequences a cluster"""
    rng = np.random.default_rng(7100 + k)
    S = 130
    names = kc.strain_names(S, "s")
    absent = tuple(names[-6:])
    recs = []
    # two distinct sequences (one chance in eight to meet under mask 0x7) beside 7 .. 40 (almost sure to)
    for i, D in enumerate((2, 2, 2, 2, 2, 2, 2, 2, 7, 20, 25, 40)):
        L = 60 + 37 * i + k
        recs.append(cluster(f"rnd{i:02d}_{D}", names, [kc.rand_seq(rng, L) for _ in range(D)], absent if i % 3 == 0 else ()))
    recs.append(cluster("tail_edge", names, a_tail_family(rng, k, 128)))          # the tails start a unit of their own
    recs.append(cluster("tail_halo", names, a_tail_family(rng, k, 84), absent))   # the tails inside the last unit
    # alleles that differ in the last base of the last word only, and in word 0 only (three words and a bit each)
    L = 32 * 3 + 32 * ((k + 31) // 32)
    base = kc.rand_seq(rng, L)
    recs.append(cluster("last_base", names, [base] + [_mut(base, [L - 1]), _mut(_mut(base, [L - 1]), [L - 1])]))
    recs.append(cluster("word0", names, [base] + [_mut(base, [p]) for p in (0, 13, 31)]))
    # identical copies only: one distinct sequence whatever the mask
    recs.append(cluster("copies_a", names, [kc.rand_seq(rng, 150 + k)]))
    recs.append(cluster("copies_b", names, [kc.rand_seq(rng, 64 + k)], absent))
    # three carriers: below the dedup pass's four segments
    recs.append(cluster("three", names, [kc.rand_seq(rng, 90 + k), kc.rand_seq(rng, 91 + k)], tuple(names[3:])))
    return dict(name=f"small_k{k}", k=k, recs=recs, names=names, stroi=(names[1], names[-1]), absent=True)


def pool_case():
    """distinct sequences that do not fit the small class's LDS pool, so that a later copy is compared with the group's
    first sequence in global memory: 12 x 12 000 bases (375 words each: under masks 0x7 and HIGH4 the sixth group's
    sequence is past the 2 048 pool words), and 2 x 66 000 bases (2 063 words: the single group of mask 0 is)"""
    rng = np.random.default_rng(7200)
    names = kc.strain_names(26, "p")
    twelve = [kc.rand_seq(rng, 12000) for _ in range(12)]
    two = [kc.rand_seq(rng, 66000) for _ in range(2)]
    assert 8 * ((12000 + 31) // 32) > POOL_WORDS_SMALL < (66000 + 31) // 32
    recs = [cluster("pool12", names, twelve), cluster("pool2", names, two, tuple(names[5:]))]
    return dict(name="pool_k31", k=31, recs=recs, names=names, stroi=(names[0],), absent=True)


# ------------------------------------------------------------------------------------------------- wide class, unit view
def _relatives(rng, founders, D, nmut=(1, 3), protect=0):
    """`founders` and descendants of theirs by one or two substitutions (not in the last `protect` bases) up to D distinct"""
    out, seen = list(founders), set(founders)
    assert len(seen) == len(out)
    while len(out) < D:
        a = out[int(rng.integers(0, len(out)))]
        b = _mut(a, [int(x) for x in rng.integers(0, len(a) - protect, int(rng.integers(*nmut)))])
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


def wide_case(k=31):
    """clusters of 66 .. 200 related distinct sequences (the table kernel unit_class_kernel, the wide dedup class)"""
    rng = np.random.default_rng(7300 + k)
    S = 232
    names = kc.strain_names(S, "w")
    absent = tuple(names[-8:])
    recs = []
    # substitutions on the unit grid
    L = 64 * 5 + k + 17
    anc = kc.rand_seq(rng, L)
    spots = sorted({0, 1, 63, 64, 65, 64 + k - 2, 64 + k - 1, 64 + k, 127, 128, 128 + k - 2, 191, 192, 2 * 64 + k - 1,
                    L - k, L - k - 1, L - 1, L - 2, 256, 255, 319, 320} & set(range(L)))
    recs.append(cluster("grid", names, _relatives(rng, [anc] + [_mut(anc, [p]) for p in spots], 70), absent))
    # truncated alleles: equal leading words, another number of bases in the last unit (nb)
    L = 64 * 4 + k + 40
    anc = kc.rand_seq(rng, L)
    cuts = [L - c for c in range(0, 45)] + [64 * 3 + k - 1, 64 * 3 + k, 64 * 2 + k + 5, 64 + k - 1, 64 + k]
    trunc = list(dict.fromkeys([anc[:c] for c in cuts] + [_mut(anc[:c], [70]) for c in cuts]))
    recs.append(cluster("trunc", names, trunc))
    # A-tails on a unit boundary and inside the last unit, among relatives of X (substitutions away from the tail)
    tails = a_tail_family(rng, k, 128) + a_tail_family(rng, k, 84)
    recs.append(cluster("tails", names, _relatives(rng, tails, 80, protect=40), absent))
    # tandem repeats whose period divides 64: units at different positions hold the same bases
    n = 64 * 4 + k + 9
    reps = [b"A" * n, b"AT" * (n // 2), (kc.rand_seq(rng, 64) * (n // 64 + 1))[:n]]
    # (first of all the 64-period repeat with a substitution in unit 0 only: its unit 1 is the first occurrence of bases that
    # the unchanged repeat, further down, holds in unit 0 as well -- position_pair_mask)
    tandem = [_mut(reps[2], [40])] + list(reps)
    for r in reps:
        tandem += [_mut(r, [p]) for p in range(3, len(r), 11)]
    tandem = list(dict.fromkeys(tandem))
    recs.append(cluster("tandem", names, tandem[:200]))
    # more unit positions than one batch of the class table takes: D = 70 -> 96 columns -> 21 unit positions a batch
    L = 64 * 23 + k + 5
    recs.append(cluster("batches", names, _relatives(rng, [kc.rand_seq(rng, L)], 70)))
    for r in recs:
        D = n_distinct(r)
        assert SMALL_MAX_D < D <= 200, (r[1], D)
    assert (64 * 23 + 5 + 63) // 64 > UNIT_PAIRS // 96
    return dict(name=f"wide_k{k}", k=k, recs=recs, names=names, stroi=(names[2],), absent=True)


def unit_contents_differ(rec, k):
    """two different unit contents anywhere in the cluster (units of 64 windows = 63 + k bases, at most): at unit-hash mask 0
    they share one class, so the cluster must keep its plain view"""
    units = set()
    for s in set(sequences(rec)):
        for u in range(0, max(len(s) - k + 1, 0), 64):
            units.add((u, s[u:u + 63 + k]))
    return len(units) >= 2


# a model of unit_class_kernel's classes: the hash of a unit, the batches of its table, which clusters must fall back
_M64 = (1 << 64) - 1


def mix64(x):
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & _M64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & _M64
    return x ^ (x >> 31)


def pack_words(seq):
    """32 bases a word, the first base in bits 63:62, A C G T = 0 1 2 3, padded with zeros"""
    out = []
    for i in range(0, len(seq), 32):
        w = 0
        for c in seq[i:i + 32]:
            w = (w << 2) | b"ACGT".index(c)
        out.append(w << 2 * (32 - len(seq[i:i + 32])))
    return out + [0, 0]


def unit_hash(seq, words, u, k):
    """(hash, nb, masked words) of the unit of 64 windows at position u, as unit_class_kernel computes them"""
    nb = min(len(seq) - 64 * u, 63 + k)
    nw = (nb + 31) // 32
    h = mix64((0x9E3779B97F4A7C15 * (nb + 1) + u) & _M64)
    content = []
    for j in range(nw):
        x = words[2 * u + j]
        if j + 1 == nw and nb & 31:
            x &= (_M64 << (64 - 2 * (nb & 31))) & _M64
        content.append(x)
        h = (mix64(h ^ x) + 0xC2B2AE3D27D4EB4F * (j + 1)) & _M64
    return h, nb, tuple(content)


def unit_fallback(rec, k, mask, position=True):
    """does unit_class_kernel leave the cluster on its plain view when the unit hash keeps the bits of `mask`: a unit that
    shares its masked hash, within one batch of the class table, with a first member of another position, nb or content.
    position=False models the kernel WITHOUT its position compare: a member is held against the first member's sequence at
    the member's own position (a first member without a unit there counts as different)."""
    seqs = list(dict.fromkeys(sequences(rec)))
    D = len(seqs)
    Dp = (D + 31) // 32 * 32
    UB = max(1, UNIT_PAIRS // Dp)
    words = [pack_words(s) for s in seqs]
    nunits = (max(map(len, seqs)) - k + 64) // 64
    for u0 in range(0, nunits, UB):
        first = {}
        for u in range(u0, min(u0 + UB, nunits)):                  # pair index order: position, then distinct index
            for d, s in enumerate(seqs):
                if 64 * u + k > len(s):
                    continue
                h, nb, content = unit_hash(s, words[d], u, k)
                fu, fd = first.setdefault(h & mask, (u, d))
                if fu != u and (position or 64 * u + k > len(seqs[fd])):
                    return True
                if unit_hash(seqs[fd], words[fd], u, k)[1:] != (nb, content):
                    return True
    return False


def nb_pair_mask(case):
    """the mask under which, of all units of the case, only the last units of X and X + 'AAAA' (tails inside the last unit:
    equal words, nb 4 apart) share a hash: every bit in which the two hashes agree"""
    k = case["k"]
    tails = next(r for r in case["recs"] if r[1] == "tails")
    seqs = list(dict.fromkeys(sequences(tails)))
    X, X4 = seqs[5], seqs[7]
    assert X4 == X + b"AAAA" and (len(X) - k) // 64 == (len(X4) - k) // 64 == 1
    (h1, nb1, c1), (h2, nb2, c2) = (unit_hash(s, pack_words(s), 1, k) for s in (X, X4))
    assert nb2 == nb1 + 4 and c1 == c2
    return ~(h1 ^ h2) & _M64


def position_pair_mask(case):
    """the mask under which only units 0 and 1 of the 64-base-period repeat (the same bases at two positions) share a hash:
    the position compare alone sends the tandem cluster back.  The cluster's first sequence is that repeat with a
    substitution in unit 0, so without the compare unit 1's piece would take the ordinal of a later sequence."""
    k = case["k"]
    tandem = next(r for r in case["recs"] if r[1] == "tandem")
    seqs = list(dict.fromkeys(sequences(tandem)))
    first, rep = seqs[0], seqs[3]
    assert rep[:64] == rep[64:128] and rep[:63 + k] == rep[64:127 + k] and len(set(rep)) == 4
    assert first[64:] == rep[64:] and first[:63 + k] != rep[:63 + k] and len(first) == len(rep)
    (h0, nb0, c0), (h1, nb1, c1) = (unit_hash(rep, pack_words(rep), u, k) for u in (0, 1))
    assert (nb0, c0) == (nb1, c1)
    return ~(h0 ^ h1) & _M64


# ------------------------------------------------------------------------------------------------- rows_kernel, mode 2
def tree_alleles(rng, D, L, nmut):
    """alleles that descend from one another: allele i is a copy of an earlier one with `nmut` substitutions, so a k-mer
    is carried by a subtree or by everything outside some subtrees: multi-bit allele masks"""
    out, seen = [kc.rand_seq(rng, L)], set()
    seen.add(out[0])
    while len(out) < D:
        b = _mut(out[int(rng.integers(0, len(out)))], [int(x) for x in rng.integers(0, L, nmut)])
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


ROWS_K = 11
ROWS_D = (65, 96, 97, 260)            # 3, 3, 4 and 9 mask words: both widths of rows_kernel's step A


def rows_case():
    rng = np.random.default_rng(7400)
    names = kc.strain_names(260, "r")
    recs = []
    for D in ROWS_D:
        # one substitution a step: few masks, many k-mers behind each; two a step at D = 260: more masks than a round's
        # table takes (MASK_TABLE_CAP), at fewer keys than one work item holds
        recs.append(cluster(f"tree{D}", names, tree_alleles(rng, D, 600 if D == 260 else 400, 2 if D == 260 else 1)))
    return dict(name=f"rows_k{ROWS_K}", k=ROWS_K, recs=recs, names=names, stroi=(), absent=False)


def mask_census(rec, k):
    """(unique canonical k-mers, distinct allele masks of two or more alleles) of a cluster"""
    carriers = {}
    for d, s in enumerate(dict.fromkeys(sequences(rec))):
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            r = kc.rc(w)
            carriers.setdefault(min(w, r), set()).add(d)
    masks = {frozenset(v) for v in carriers.values() if len(v) >= 2}
    return len(carriers), len(masks)


# ------------------------------------------------------------------------------------------------- the runs
def cases():
    return [small_case(k) for k in SMALL_K] + [pool_case(), wide_case(), rows_case()]


def runs(case):
    """(sites, mask, consider_missing) of a case; sites None = every site"""
    out = []
    cms = (False, True) if case["absent"] else (False,)
    for cm in cms:
        out += [(None, m, cm) for m in MASKS]
        if case["name"].startswith("wide"):
            out.append((None, WIDE_MASK, cm))
        if case["name"].startswith(("wide", "rows")):
            # the unit-class and mask-table compares see only clusters whose dedup pass met no collision: that hash whole
            out += [(site, m, cm) for site in (SITE_UNIT, SITE_ROWS) for m in MASKS[1:]]
        if case["name"].startswith("wide") and not cm:
            out.append((SITE_UNIT, nb_pair_mask(case), cm))     # the nb compare as the only thing between two units
            out.append((SITE_UNIT, position_pair_mask(case), cm))    # ... and the position compare
    return out


def run_id(case, run):
    sites, mask, cm = run
    site = {None: "all", SITE_UNIT: "unit", SITE_ROWS: "rows"}[sites]
    return f"{case['name']}-{site}-{mask:#x}-{'missing' if cm else 'present'}"


def engine_options(case, cm):
    S = len(case["names"])
    return dict(klength=case["k"], canon=True, consider_missing=cm, max_strains=(S + 31) // 32 * 32, stroi=set(case["stroi"]),
                max_items=64)


# ------------------------------------------------------------------------------------------------- N5: the plot grid
def plot_table(two_clusters=False, n_rows=6000, seed=11):
    """an annotated k-mer table of one cluster name and one p-value text (or two names); strains s0 .. s44 of which s0 .. s39
    are phenotype strains"""
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 45, n_rows)
    pos = rng.integers(-12, 40, n_rows)
    kmer = np.array(["ACGT", "cGTA", "NNAC", "TTga", "GAtc"])[rng.integers(0, 5, n_rows)]
    strand = np.where(rng.random(n_rows) < 0.5, -1, 1)
    lines = ["cluster\tk-mer\tlrt-pvalue\tstrain\tgene_start\tstrand"]
    for i in range(n_rows):
        cl = "g1" if two_clusters and i % 2 else "g0"
        lines.append(f"{cl}\t{kmer[i]}\t1e-3\ts{st[i]}\t{pos[i]}\t{strand[i]}")
    return "\n".join(lines) + "\n", [f"s{i}" for i in range(40)], [0, 3, 4, 1, 5, 2]
