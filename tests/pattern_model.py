"""Test-side models that need neither the GPU, the oracle nor the library.

`check_rows`: the plain reference of the hashing and text kernels.  Given the headerless texts of
`hashes_to_patterns.tsv` and `kmers_to_hashes.tsv` it rebuilds every row's vector from the row's own cells and
re-hashes it the way the reference does (panfeed.py:175-176, 206-207): base64(md5(vector.view(uint8)))[:24].
A k-mer's row is the float64 image ('' = NaN).  A cluster's own row -- the hash a `kmers_to_hashes` line with an
empty k-mer field names -- is the image of `clusterpresab`, which the reader makes with dtype=int (input.py:375) and
pattern_hasher hashes as it comes (panfeed.py:175): int64, with and without --consider-missing-cluster, and its cells
are never empty (panfeed.py:184-186: an int is never NaN).

`count_exact_cluster`: one cluster of S strains whose k-mer presence counts are chosen, so that the number of rows
the MAF cut keeps follows from panfeed.py:190-200 alone (`kept_rows`).
"""
import binascii
import hashlib
import math

import numpy as np

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def digest(vec):
    """panfeed.py:175-176 / 206-207"""
    return binascii.b2a_base64(hashlib.md5(np.ascontiguousarray(vec).view(np.uint8)).digest()).decode()[:24]


def _lines(text):
    assert text == "" or text.endswith("\n"), "text does not end with a newline"
    return text.split("\n")[:-1]


def check_rows(hashes_to_patterns, kmers_to_hashes, n_strains, consider_missing, known=None):
    """Every row of `hashes_to_patterns` has exactly `n_strains` cells and re-hashes to its own name; every hash
    `kmers_to_hashes` names has a row, here or among `known` (the run-global pattern set before these texts, panfeed.py
    :149-150); no row is written twice and none without a line that names it.  Returns `known` plus the new rows' hashes."""
    known = set() if known is None else set(known)
    named, own = [], set()
    for ln in _lines(kmers_to_hashes):
        f = ln.split("\t")
        assert len(f) == 3, f"kmers_to_hashes line with {len(f)} fields: {ln[:80]!r}"
        assert len(f[2]) == 24, f"hash of {len(f[2])} characters: {ln[:80]!r}"
        named.append(f[2])
        if f[1] == "":
            own.add(f[2])
    new = set()
    for ln in _lines(hashes_to_patterns):
        name, _, rest = ln.partition("\t")
        cells = rest.split("\t")
        assert len(cells) == n_strains, f"row {name}: {len(cells)} cells for {n_strains} strains"
        assert name not in known and name not in new, f"row {name} written twice"
        bad = sorted(set(cells) - {"0", "1", ""})
        assert not bad, f"row {name}: cells {bad[:5]}"
        empty = np.array([c == "" for c in cells], dtype=bool)
        ones = np.array([c == "1" for c in cells], dtype=bool)
        as_int = ones.astype(np.int64)
        as_float = ones.astype(np.float64)
        as_float[empty] = np.nan
        if name in own:
            assert not empty.any(), f"cluster row {name} has empty cells"
            got, kind, other = digest(as_int), "int64", digest(as_float)
        else:
            assert consider_missing or not empty.any(), f"row {name} has empty cells without consider_missing"
            got, kind, other = digest(as_float), "float64", digest(as_int)
        assert got == name, (f"row {name} ({n_strains} cells, {int(ones.sum())} ones, {int(empty.sum())} empty): its {kind} "
                             f"image hashes to {got}" + (f"; the name is the digest of the other image" if other == name else
                                                         ": the digest does not belong to these bits"))
        new.add(name)
    have = known | new
    missing = [h for h in named if h not in have]
    assert not missing, f"{len(missing)} hashes of kmers_to_hashes without a row, first {missing[0]}"
    unnamed = new - set(named)
    assert not unnamed, f"{len(unnamed)} rows no kmers_to_hashes line names, first {sorted(unnamed)[0]}"
    return have


# ----------------------------------------------------------------------------------------------- generators
def _seqinfo(seq, sid, chrom, start, strand, offset):
    from panfeed_amd.classes import Seqinfo
    return Seqinfo(seq.decode(), seq.translate(_COMP).decode(), sid, chrom, start, start + len(seq) - 1, strand, offset)


def _canon(b):
    r = b.translate(_COMP)[::-1]
    return min(b, r)


def strain_names(S):
    """names whose sorted order is the column order"""
    return [f"s{i:05d}" for i in range(S)]


class CountExact:
    """what count_exact_cluster made: `record` (gene_sequences, idx, clusterpresab), `names` (column order), `present`
    (columns with the cluster), `kmer_counts` (presence count of every distinct canonical k-mer)"""

    def __init__(self, record, names, present, kmer_counts, S):
        self.record, self.names, self.present, self.kmer_counts, self.S = record, names, present, kmer_counts, S


def count_exact_cluster(S, k, counts, seed, idx="cx", n_absent=0, keep_present=()):
    """A base sequence with one substitution per entry of `counts`, at positions k + 1 apart, each carried by exactly
    counts[j] of the present strains (a seeded permutation of the columns picks them): every c = counts[j] gives k
    k-mers of count c and k of count P - c (P = present strains), the other windows have count P.  `n_absent` columns
    (never those of `keep_present`) are without the cluster.  The dict is filled in a seeded order of its own."""
    rng = np.random.default_rng(seed)
    names = strain_names(S)
    cols = rng.permutation(S)
    keep = set(int(c) % S for c in keep_present)
    cols = np.array([c for c in cols if int(c) not in keep] + sorted(keep), dtype=np.int64)   # kept columns last
    assert n_absent <= S - max(1, len(keep))
    absent, present = cols[:n_absent], cols[n_absent:]
    P = len(present)
    counts = [int(c) for c in counts]
    assert all(1 <= c <= P - 1 for c in counts), (counts, P)
    J = len(counts)
    gap = k + 1
    L = 2 * k + max(J - 1, 0) * gap + 1
    pos = [k + j * gap for j in range(J)]
    while True:
        base = rng.integers(0, 4, L)
        alt = [(base[p] + 1 + int(rng.integers(0, 3))) & 3 for p in pos]
        # every window, with and without its substitution, must be a k-mer of its own (counts would add up otherwise)
        kmers = {}
        full = base.copy()
        for p, a in zip(pos, alt):
            full[p] = a
        for w in range(L - k + 1):
            hit = [j for j, p in enumerate(pos) if w <= p < w + k]
            assert len(hit) <= 1
            b0 = _canon(_ACGT[base[w:w + k]].tobytes())
            if not hit:
                kmers.setdefault(b0, []).append(P)
            else:
                kmers.setdefault(b0, []).append(P - counts[hit[0]])
                kmers.setdefault(_canon(_ACGT[full[w:w + k]].tobytes()), []).append(counts[hit[0]])
        if all(len(v) == 1 for v in kmers.values()):
            break
    carriers = np.zeros((J, S), dtype=bool)
    for j, c in enumerate(counts):
        carriers[j, rng.permutation(present)[:c]] = True
    presab = np.zeros(S, dtype=np.int64)
    presab[present] = 1
    cache = {}
    gs = {}
    for i in rng.permutation(S):
        i = int(i)
        if not presab[i]:
            gs[names[i]] = []
            continue
        key = carriers[:, i].tobytes()
        if key not in cache:
            s = base.copy()
            for j in range(J):
                if carriers[j, i]:
                    s[pos[j]] = alt[j]
            cache[key] = _ACGT[s].tobytes()
        gs[names[i]] = [_seqinfo(cache[key], f"{names[i]}_{idx}", f"{names[i]}_c", 100 + 3 * i, 1 if i % 3 else -1, 0)]
    return CountExact((gs, idx, presab), names, P, [v[0] for v in kmers.values()], S)


def maf_keeps(count, n, maf):
    """panfeed.py:190-200 in Python floats"""
    af = count / n
    if af >= .5:
        af = 1 - af
    return not af < maf


def kept_rows(cx, maf, consider_missing):
    """k-mer rows of kmers_to_hashes.tsv the MAF cut leaves of a CountExact cluster (patfilt=True): the denominator is
    the row's length, or its non-NaN cells with consider_missing (panfeed.py:191, 194-196)"""
    n = cx.present if consider_missing else cx.S
    return sum(1 for c in cx.kmer_counts if maf_keeps(c, n, maf))


def edge_counts(S, maf):
    """the issue's count list for S strains and a MAF: 1, S-1; floor(maf S) - 1, floor(maf S), ceil(maf S),
    ceil(maf S) + 1 and their complements; S/2; (S +- 1)/2 when S is odd -- those that a substitution can carry
    (1..S-1), one of each complementary pair (a substitution of count c brings the k-mers of count S - c along)"""
    lo, hi = math.floor(maf * S), math.ceil(maf * S)
    want = [1, S - 1, lo - 1, lo, hi, hi + 1, S - (lo - 1), S - lo, S - hi, S - (hi + 1)]
    want += [(S - 1) // 2, (S + 1) // 2] if S % 2 else [S // 2]
    out = []
    for c in want:
        if 1 <= c <= S - 1 and c not in out and S - c not in out:
            out.append(c)
    return out
