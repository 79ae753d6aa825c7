"""K-mer content the random generators never make, and a model of what the reference does with it.  No GPU, no
oracle, no library: numpy and str only.

Generators (each returns a list of (kind, sequence) alleles; `cluster` deals them to samples round robin):
near-palindromes `flank + X + rc(X) + flank` with one substitution in the right arm per chosen first-difference base,
exact palindromes, homopolymers and tandem repeats longer than two 64-window units, sequences that differ only by
trailing 'A's (which pack to the same bits as padding), a sequence beside its reverse complement, and a cluster whose
first distinct sequences are tandem repeats and whose later ones are unique.

`model_clusters` restates the reference's cluster_cutter (panfeed.py:45-107) with a dict and str comparison and
classifies every window by the 63-bit key word in which the forward and the reverse-complement value first differ;
`check_kmers` holds a run's three texts against it.
"""
from collections import Counter

import numpy as np

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def rc(b):
    return b.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def key_words(k):
    """63-bit words of a k-mer's key: k <= 31 one, <= 63 two, <= 94 three, <= 126 four"""
    return (2 * k + 62) // 63


# ----------------------------------------------------------------------------------------------- generators
def first_difference_bases(k):
    """bases p at which a near-palindrome's two strands are made to differ first: the first base, the bases on either
    side of bit 63 of the value, the last pair before the centre"""
    return [p for p in dict.fromkeys((0, 31, 32, k // 2 - 1)) if 0 <= p < k // 2]


def palindromes(rng, k, flank=9):
    """Two families `flank + X + mid + rc(X) + flank` (mid: one base when k is odd, so that the centred window pairs
    every base but its middle one with its complement).  X carries a 'C' (family 0) or a 'G' (family 1) at each chosen
    first-difference base p of the centred window, and a copy per p substitutes the paired base of the right arm --
    k/2 - 1 - p bases past the centre -- so that the reverse complement shows another base at p:
      family C:  A there (only the low bit differs, reverse smaller)   T there at p = 31 (the high bit, forward smaller)
      family G:  T there (only the low bit differs, forward smaller)   A there at p = 31 (the high bit, reverse smaller)
    The unmodified sequences hold one exactly palindromic window each when k is even."""
    out = []
    m = max(k, 8) + 3
    ps = first_difference_bases(k)
    for fam, left in enumerate("CG"):
        f0, f1 = rand_seq(rng, flank), rand_seq(rng, flank + 2 * fam)
        X = bytearray(rand_seq(rng, m))
        mid = rand_seq(rng, 1) if k % 2 else b""
        s = (2 * m + len(mid) - k) // 2                      # start of the centred window within X + mid + rc(X)
        for p in ps:
            X[s + p] = ord(left)
        core = bytes(X) + mid + rc(bytes(X))
        out.append((f"pal{fam}", f0 + core + f1))
        for p in ps:
            shows = {"C": "AT", "G": "TA"}[left] if p == 31 else {"C": "A", "G": "T"}[left]
            for y in shows:
                b = bytearray(core)
                assert b[s + k - 1 - p] == ord(rc(left.encode()))
                b[s + k - 1 - p] = rc(y.encode())[0]         # the reverse complement shows y at base p
                out.append((f"pal{fam}_p{p}{y}", f0 + bytes(b) + f1))
    return out


def at_repeat(k):
    """(AT)n: every window of an even k is its own reverse complement; two units and a bit"""
    return b"AT" * ((2 * 64 + k + 7) // 2 + 1)


def repeats(rng, k):
    n = 2 * 64 + k + 5                                       # whole 64-window units of one key
    unit7, unit64 = rand_seq(rng, 7), rand_seq(rng, 64)
    mid = b"ACG" * ((64 + k) // 3 + 2)
    return [("rep_A", b"A" * n), ("rep_T", b"T" * n), ("rep_AT", at_repeat(k)),
            ("rep_ACG", b"ACG" * (n // 3 + 1)), ("rep_7", unit7 * (n // 7 + 1)), ("rep_64", (unit64 * (n // 64 + 2))[:n + 64]),
            ("rep_mid", rand_seq(rng, 40 + k) + mid + rand_seq(rng, 30 + k))]


def a_tails(rng, k):
    """X, X + 'A', X + 'AAAA', X + 33 'A' (one more packed word) and X without its last base, where X ends in 'A':
    once with X ending on a unit boundary (128 windows: any longer allele starts a unit of its own), once with the
    tails inside the last unit (84 windows); a sequence of exactly k bases and one of k - 1"""
    out = []
    for tag, nwin, tails in (("edge", 128, (1, 4, 33)), ("halo", 84, (1, 4))):
        X = rand_seq(rng, nwin + k - 2) + b"CA"              # X[:-1] ends in 'C': its last base is no padding
        out.append((f"tail_{tag}", X))
        out += [(f"tail_{tag}+{t}", X + b"A" * t) for t in tails]
        out.append((f"tail_{tag}-1", X[:-1]))
    Y = rand_seq(rng, k)
    out.append(("len_k", Y))
    if k > 1:
        out.append(("len_k-1", Y[:-1]))
    return out


def rc_pair(rng, k):
    X = rand_seq(rng, 3 * 64 + k + 11)
    return [("fwd", X), ("rc", rc(X))]


def palindrome_alleles(rng, k):
    """the alleles of the first cluster: both palindrome families, (AT)n, a sequence and its reverse complement"""
    return palindromes(rng, k) + [("rep_AT", at_repeat(k))] + rc_pair(rng, k)


def repeat_alleles(rng, k):
    """the alleles of the second cluster: repeats and A-tails"""
    return repeats(rng, k) + a_tails(rng, k)


def _distinct(alleles):
    seen, out = set(), []
    for kind, s in alleles:
        if s not in seen:
            seen.add(s)
            out.append((kind, s))
    return out


def strain_names(S, prefix="c"):
    return [f"{prefix}{i:03d}" for i in range(S)]


def cluster(idx, names, alleles, copies=3):
    """a reference-shaped record: sample i carries allele i mod D (at least `copies` samples per allele, so that the
    identical-sequence shortcut and the unit view apply), strands alternate"""
    from panfeed_amd.classes import Seqinfo
    seqs = [s for _, s in alleles]
    assert len(names) >= copies * len(seqs), (len(names), len(seqs))
    gs, presab = {}, np.zeros(len(names), dtype=np.int64)
    col = {x: i for i, x in enumerate(sorted(names))}
    for i, nm in enumerate(names):
        sq = seqs[i % len(seqs)]
        gs[nm] = [Seqinfo(sq.decode(), sq.translate(_COMP).decode(), f"{nm}_{idx}", f"{nm}_c", 50 + i, 50 + i + len(sq) - 1,
                          1 if i % 2 else -1, 0)]
        presab[col[nm]] = 1
    return gs, idx, presab


def content_clusters(k, seed=0, absent=0):
    """the cluster pair of one k: (records, names, kinds) with kinds[cluster][kind] = the first sample that carries
    it.  `absent` strains (the last names) are without the second cluster."""
    rng = np.random.default_rng(1000 * seed + k)
    pal, rep = _distinct(palindrome_alleles(rng, k)), _distinct(repeat_alleles(rng, k))
    S = 3 * max(len(pal), len(rep)) + 2
    names = strain_names(S)
    recs = [cluster("g_pal", names, pal), cluster("g_rep", names, rep)]
    if absent:
        gs, idx, presab = recs[1]
        col = {x: i for i, x in enumerate(sorted(names))}
        for nm in names[-absent:]:
            gs[nm] = []
            presab[col[nm]] = 0
    kinds = [{kind: names[i] for i, (kind, _) in enumerate(al)} for al in (pal, rep)]
    return recs, names, kinds


def back_loaded_cluster(n_repeat, n_unique, length, head, seed=0, idx="g_back", copies=3):
    """D = n_repeat + n_unique distinct sequences of `length` bases.  The first are a tandem repeat of a motif of their
    own (a handful of keys each, no unit in common); the later ones begin with `head` bases of such a repeat and go on
    as unique random sequence (`length - head` keys each).  New keys come late whether the sequences are walked one
    after the other or position by position."""
    rng = np.random.default_rng(seed)

    def tandem(n):
        motif = rand_seq(rng, int(rng.integers(5, 10)))
        return (motif * (n // len(motif) + 1))[:n]

    alleles = [(f"back_rep{i}", tandem(length)) for i in range(n_repeat)]
    alleles += [(f"back_uni{i}", tandem(head) + rand_seq(rng, length - head)) for i in range(n_unique)]
    alleles = _distinct(alleles)
    assert len(alleles) == n_repeat + n_unique
    names = strain_names(copies * len(alleles), "b")
    return cluster(idx, names, alleles, copies), names


# ----------------------------------------------------------------------------------------------- model
def classify(spec, rev, k):
    """where `spec` and `rev` first differ: None for a tie, else (word, reverse_smaller, base, low_bit_only).  The key
    is the 2k-bit value (first base most significant, two bits a base) right-aligned in key_words(k) words of 63 bits,
    most significant first: bit b from the top is bit 2k - 1 - b of the value, in word KW - 1 - (2k - 1 - b) // 63."""
    if spec == rev:
        return None
    p = next(i for i in range(k) if spec[i] != rev[i])
    a, b = _CODE[spec[p]], _CODE[rev[p]]
    low_only = not ((a ^ b) & 2)
    bit = 2 * p + (1 if low_only else 0)
    word = key_words(k) - 1 - (2 * k - 1 - bit) // 63
    return word, b < a, p, low_only


class ClusterModel:
    """`kmers`: k-mer -> set of sample columns, in insertion order; `rows`: the kmers.tsv lines of the target strains;
    `classes`: Counter of classify() over every window; `one_key_units`: 64-window units whose windows share one
    canonical k-mer; `equal_pairs`: windows whose forward and reverse-complement k-mers are the same string"""

    def __init__(self, idx, n_strains, presab):
        self.idx, self.n_strains, self.presab = idx, n_strains, presab
        self.kmers, self.rows, self.classes, self.one_key_units, self.equal_pairs = {}, [], Counter(), 0, 0


def _windows(seq, comp, k, cache):
    key = (seq, comp)
    if key not in cache:
        w = []
        for pos in range(len(seq) - k + 1):
            spec = seq[pos:pos + k]                          # panfeed.py:65
            rev = comp[pos:pos + k][::-1]                    # panfeed.py:67
            w.append((spec, rev, classify(spec, rev, k) if "N" not in spec else None))
        cache[key] = w
    return cache[key]


def model_clusters(records, k, canon, stroi=()):
    """panfeed.py:45-107 in plain Python, one ClusterModel per record"""
    out, cache = [], {}
    for gs, idx, presab in records:
        col = {x: i for i, x in enumerate(sorted(gs.keys()))}                    # :47-48
        m = ClusterModel(idx, len(col), np.asarray(presab))
        counted = set()
        for strain in gs.keys():                                                  # :54
            for s in gs[strain]:
                wins = _windows(s.sequence, s.compsequence, k, cache)
                if (s.sequence, s.compsequence) not in counted:                   # statistics: once per distinct sequence
                    counted.add((s.sequence, s.compsequence))
                    canons = []
                    for spec, rev, cls in wins:
                        m.classes[cls] += 1
                        m.equal_pairs += spec == rev
                        canons.append(spec if spec <= rev else rev)
                    for u in range(len(canons) // 64):
                        m.one_key_units += len(set(canons[64 * u:64 * u + 64])) == 1
                for pos, (spec, rev, _) in enumerate(wins):
                    if canon:
                        canonseq, used = (spec, 1) if spec <= rev else (rev, -1)  # :70-75
                        m.kmers.setdefault(canonseq, set()).add(col[strain])
                    else:
                        used = s.strand                                           # :81
                        m.kmers.setdefault(spec, set()).add(col[strain])
                        m.kmers.setdefault(rev, set()).add(col[strain])
                    if strain in stroi:                                           # :90-107
                        if s.strand > 0:
                            t0, t1 = s.start + pos, s.start + pos + k
                        else:
                            t0, t1 = s.end - pos - k, s.end - pos
                        head = f"{idx}\t{strain}\t{s.id}\t{s.chromosome}\t{s.strand}\t{t0}\t{t1}\t{pos - s.offset}\t{pos + k - s.offset}"
                        if canon:
                            m.rows.append(f"{head}\t{used}\t{canonseq}")
                        else:
                            m.rows.append(f"{head}\t{used}\t{spec}")
                            m.rows.append(f"{head}\t{-used}\t{rev}")
        out.append(m)
    return out


def _lines(text):
    assert text == "" or text.endswith("\n"), "text does not end with a newline"
    return text.split("\n")[:-1]


def _body(text, header):
    """the text without its header line, when it has one"""
    return text[text.index("\n") + 1:] if text.startswith(header) else text


def check_kmers(kmers_to_hashes, hashes_to_patterns, kmers_tsv, records, k, canon, stroi=(), consider_missing=False,
                patfilt=True, models=None):
    """A run's texts (with or without their header lines) against the model, for a run with maf = 0.0: the k-mers of
    every cluster in the order the reference's dict holds them, each k-mer's row -- through the hash its line names --
    against its sample set, and every line of kmers.tsv.  With patfilt=False the reference leaves out the k-mers whose
    row equals the cluster's own (panfeed.py:202-204); the model does the same.  Returns the models."""
    models = model_clusters(records, k, canon, stroi) if models is None else models
    rows = {}
    for ln in _lines(_body(hashes_to_patterns, "hashed_pattern")):
        name, _, rest = ln.partition("\t")
        assert name not in rows, f"row {name} written twice"
        rows[name] = rest.split("\t")
    got = {}
    order = []
    for ln in _lines(_body(kmers_to_hashes, "cluster\t")):
        idx, kmer, h = ln.split("\t")
        if kmer == "":
            assert idx not in got, f"cluster {idx} twice"
            got[idx] = []
            order.append(idx)
        else:
            assert order and order[-1] == idx, f"k-mer line of {idx} outside its cluster"
            got[idx].append((kmer, h))
    assert order == [m.idx for m in models], "clusters of kmers_to_hashes"
    for m in models:
        present = set(int(i) for i in np.flatnonzero(m.presab))
        whole = len(m.presab) == m.n_strains and not (consider_missing and len(present) < m.n_strains)
        expect = [(km, cols) for km, cols in m.kmers.items() if patfilt or not (whole and cols == present)]
        gk = [km for km, _ in got[m.idx]]
        ek = [km for km, _ in expect]
        if gk != ek:
            i = next((i for i, (a, b) in enumerate(zip(gk, ek)) if a != b), min(len(gk), len(ek)))
            raise AssertionError(f"cluster {m.idx}: {len(gk)} k-mers for {len(ek)}; at {i}: "
                                 f"{gk[i] if i < len(gk) else None!r} for {ek[i] if i < len(ek) else None!r}")
        for (km, h), (_, cols) in zip(got[m.idx], expect):
            assert h in rows, f"cluster {m.idx}: {km} names {h}, which has no row"
            cells = ["1" if c in cols else ("" if consider_missing and c < len(m.presab) and not m.presab[c] else "0")
                     for c in range(m.n_strains)]
            assert rows[h] == cells, (f"cluster {m.idx}: the row of {km} ({h}) has ones at "
                                      f"{[i for i, c in enumerate(rows[h]) if c == '1'][:12]}, the model at {sorted(cols)[:12]}")
    gt = _lines(_body(kmers_tsv, "cluster\tstrain"))
    et = [r for m in models for r in m.rows]
    if gt != et:
        i = next((i for i, (a, b) in enumerate(zip(gt, et)) if a != b), min(len(gt), len(et)))
        raise AssertionError(f"kmers.tsv: {len(gt)} lines for {len(et)}; line {i}: "
                             f"{gt[i] if i < len(gt) else None!r} for {et[i] if i < len(et) else None!r}")
    return models
