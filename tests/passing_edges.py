"""Edges of the passing-rows filter (pass_mark_kernel, kt_row_passes, the FILTER kernels, kt_filter_prepare,
passing_build_set): inputs on which single rows pass or fail, the filter stated on text alone, and the conditions that
keep every case on its edge.  No GPU, no library: the CPU oracle, numpy and str only.

* `fragment_cluster`: a target strain carries a random X of nwin + k - 1 bases, fragment strain j carries
  X[a_j : b_j + k - 1].  Windows a_j .. b_j - 1 of the target have the pattern {target, j}, which has a hash of its own;
  every other window has {target}.  A passing list of some of those hashes keeps exactly the chosen row ranges.
  `geometry` places the ranges on the seams of the row kernels' tiles (KT_ROWS rows) and waves (64 rows) and the
  coordinates where the digit counts change; `fragment_case` holds every list's claimed row indices.
* `arena_batch`: a cluster that overflows its scan table twice between two small ones.
* `grow_case`: a pangenome of the kind of passing_cases with more patterns than a 512-pattern pool, for a run in batches.
* `wrap_index` / `wrap_set`: restatements of pass_mix64, pass_digest_hash and pass_key_hash, a cluster whose index
  chains wrap past the last slot and a passing list whose set chains do.  The GPU test reads the device's tables back
  and holds them against these; a wrong restatement fails there, it cannot lose coverage quietly.
* `content_case`: kmer_content.content_clusters under a list that splits the palindromes, the (AT)n pairs, the
  fwd / rc strains and keeps a tile of the homopolymer whole.

The filter is always: the oracle's kmers.tsv rows whose (field 1, field 11) the oracle's kmers_to_hashes lists with a
hash of the list (`filter_rows`).  No generator is trusted: tests/test_passing_edges.py recomputes every claim."""
import base64
import collections
import functools

import numpy as np

import kmer_content as kc

KT_ROWS = 256                  # pf_kernels.h: rows per tile of the row kernels; a wave is 64 of them
MASK64 = (1 << 64) - 1
ALL, TARGET = "every hash", "the hash of {target}"

# every seam the issue names; each is claimed by at least one case (test_passing_edges.py holds the list against the cases)
EDGES = (["only_row_0", "only_last_row", "only_last_row_of_a_tile", "only_first_row_of_a_tile", "both_rows_of_a_tile_seam",
          "rows_63_64_of_a_wave", "waves_dropped", "only_wave_2", "tile_empty_between_two_kept", "tile_kept_between_two_empty",
          "every_hash", "target_hash_only", "digits_differ_across_a_dropped_stretch",
          "last_tile:1", "last_tile:255", "last_tile:256",
          "contig_start_5_digits_at_the_seam", "contig_end_4_digits_at_the_seam", "gene_start_changes_sign_in_a_kept_range"] +
         [f"key_width:k{k}:{m}" for k in (31, 32, 63, 64, 94, 95, 126) for m in ("canon", "both")] +
         ["arenas:retried_between_two_small", "batches:pattern_table_grows", "batches:pattern_of_batch_1_in_a_later_batch",
          "wrap:index_present", "wrap:index_absent", "wrap:set_present", "wrap:set_absent", "set:fillers_only"] +
         [f"content:{c}:{m}" for c in ("palindrome", "second_word", "fwd_rc", "rep_A_tile") for m in ("canon", "both")] +
         ["content:at_pairs:both"])


def oracle_texts(records, **kw):
    from oracle import oracle as po
    run = po.OracleRun(**kw)
    run.feed(records)
    return run.texts()


def text_of(rows):
    return "".join(r + "\n" for r in rows)


class Texts:
    """the oracle's side of a batch: kt / kh / hp, the rows of kt, the (cluster, k-mer) -> hash pairs of kh, the
    distinct hashes in file order"""

    def __init__(self, kt, kh, hp):
        self.kt, self.kh, self.hp = kt, kh, hp
        self.rows = kt.split("\n")[:-1]
        self.pairs, hashes = {}, {}
        for line in kh.split("\n"):
            if line:
                idx, kmer, h = line.split("\t")
                if kmer:
                    self.pairs[(idx, kmer)] = h
                    hashes[h] = None
        self.hashes = list(hashes)
        self.row_hash = [self.pairs.get((r.split("\t", 1)[0], r.rsplit("\t", 1)[1])) for r in self.rows]

    def kept(self, passing):
        """the contract: indices of the rows whose pair kmers_to_hashes lists with a hash of `passing`"""
        passing = set(passing)
        return [i for i, h in enumerate(self.row_hash) if h in passing]

    def filter_rows(self, passing):
        return [self.rows[i] for i in self.kept(passing)]

    def filtered(self, passing):
        return text_of(self.filter_rows(passing))


def seq_key(row):
    return tuple(row.split("\t", 3)[:3])


def tile_units(rows, kept, reps_rows_per_seq):
    """bytes of every tile of the device text under `kept` (indices into `rows`): the rows of one sequence, KT_ROWS at a
    time.  reps_rows_per_seq: {sequence key: its row count}, in text order"""
    units, at = [], 0
    keep = set(kept)
    for key, n in reps_rows_per_seq.items():
        for r0 in range(0, n, KT_ROWS):
            units.append(sum(len(rows[at + i]) + 1 for i in range(r0, min(n, r0 + KT_ROWS)) if at + i in keep))
        at += n
    return units


def ranges_at_smallest_budget(units):
    """kt_plan at the budget 2 * (largest unit + 64): one range where the whole text (and its 64 bytes of slack) fits
    that; else a range closes before the unit that would take it past the largest unit"""
    cap, cur, n = max(units, default=0), 0, 0
    if sum(units) + 64 <= 2 * (cap + 64):
        return 1 if sum(units) else 0
    for u in units:
        if cur and cur + u > cap:
            n, cur = n + 1, 0
        cur += u
    return n + (1 if cur else 0)


# ----------------------------------------------------------------------------------------------- 1. the fragment cluster
def fragment_cluster(k, nwin, frags, strand=1, start=50, offset=0, seed=0, idx="g_frag"):
    """(record, names): names[0] the target, names[1 + j] the carrier of windows frags[j] = (a, b)"""
    from panfeed_amd.classes import Seqinfo
    rng = np.random.default_rng(seed)
    X = kc.rand_seq(rng, nwin + k - 1)
    names = ["t000"] + [f"f{j:03d}" for j in range(len(frags))]
    seqs = [X] + [X[a:b + k - 1] for a, b in frags]
    assert all(0 <= a < b <= nwin for a, b in frags)
    gs = {}
    for i, (nm, s) in enumerate(zip(names, seqs)):
        st, sd, off = (start, strand, offset) if i == 0 else (50 + i, 1, 0)
        gs[nm] = [Seqinfo(s.decode(), s.translate(kc._COMP).decode(), f"{nm}_g", f"{nm}_c", st, st + len(s) - 1, sd, off)]
    return (gs, idx, np.ones(len(names), dtype=np.int64)), names


class Geometry:
    """rows(reps) -> total rows; frags: name -> (first row, row behind the last), multiples of reps (rows per window);
    lists: name -> (fragment names | ALL | TARGET, the edges the list stands on)"""

    def __init__(self, name, nrows, frags, strand, coord, offset, lists, edges):
        self.name, self.nrows, self.frags, self.strand, self.coord, self.offset = name, nrows, frags, strand, coord, offset
        self.lists, self.edges = lists, edges


def geometry(name, reps):
    """the row ranges of geometry `name` where a window makes `reps` rows (1 canonical, 2 not)"""
    R, T = reps, KT_ROWS
    # the first five-digit contig_start is row 255 (canonical) or the window of rows 256 / 257; contig_end drops to four
    # digits there on the reverse strand
    fwd, rev = 10_000 - (255 if R == 1 else 128), 10_000 + (254 if R == 1 else 127)
    if name == "seams":            # three whole tiles and a last tile of one window
        frags = dict(r0=(0, R), w63=(64 - R, 64 + R), r255=(T - R, T), r256=(T, T + R), wave2=(T + 128, T + 192),
                     tile2=(2 * T, 3 * T), last=(3 * T, 3 * T + R))
        lists = dict(row0=(["r0"], ["only_row_0"]), last=(["last"], ["only_last_row"]),
                     r255=(["r255"], ["only_last_row_of_a_tile"]), r256=(["r256"], ["only_first_row_of_a_tile"]),
                     r255_256=(["r255", "r256"], ["both_rows_of_a_tile_seam"]),
                     r63_64=(["w63"], ["rows_63_64_of_a_wave", "waves_dropped"]),
                     wave2=(["wave2"], ["only_wave_2", "waves_dropped", "gene_start_changes_sign_in_a_kept_range"]),
                     across=(["w63", "wave2", "last"], ["digits_differ_across_a_dropped_stretch"]),
                     every=(ALL, ["every_hash"]), target=(TARGET, ["target_hash_only"]))
        return Geometry(name, 3 * T + R, frags, 1, fwd, (T + 144) // R, lists,
                        ["last_tile:1", "contig_start_5_digits_at_the_seam"])
    if name == "tiles":            # a last tile one window short of whole
        frags = dict(tile0=(0, T), tile2=(2 * T, 3 * T - R))
        lists = dict(tiles02=(["tile0", "tile2"], ["tile_empty_between_two_kept", "gene_start_changes_sign_in_a_kept_range"]),
                     every=(ALL, ["every_hash"]), target=(TARGET, ["target_hash_only", "tile_kept_between_two_empty"]))
        return Geometry(name, 3 * T - R, frags, -1, rev, 100 // R, lists, ["last_tile:255", "contig_end_4_digits_at_the_seam"])
    if name == "two":              # two whole tiles: the key-width sweep's batch
        frags = dict(r255=(T - R, T), r256=(T, T + R), last=(2 * T - R, 2 * T))
        lists = dict(seams3=(["r255", "r256", "last"], ["both_rows_of_a_tile_seam", "only_last_row"]),
                     target=(TARGET, ["target_hash_only"]))
        return Geometry(name, 2 * T, frags, 1, fwd, 0, lists, ["last_tile:256", "contig_start_5_digits_at_the_seam"])
    raise KeyError(name)


SWEEP_K = (31, 32, 63, 64, 94, 95, 126)
# (geometry, k, canonical): the seams at the first and last k of a key width; the sweep's batch at every such k
FRAGMENT_CASES = ([("seams", 31, True), ("seams", 32, False), ("seams", 95, True), ("tiles", 31, True), ("tiles", 32, False)] +
                  [("two", k, canon) for k in SWEEP_K for canon in (True, False)])


class FragmentCase:
    """one batch: the record, its oracle texts, and per list (hashes, claimed row indices, edges)"""

    def __init__(self, geo, k, canon):
        reps = 1 if canon else 2
        g = self.geo = geometry(geo, reps)
        self.name, self.k, self.canon, self.reps = f"{geo}-k{k}-{'canon' if canon else 'both'}", k, canon, reps
        self.fnames = list(g.frags)
        frags = [(g.frags[f][0] // reps, g.frags[f][1] // reps) for f in self.fnames]
        assert all(r % reps == 0 for f in self.fnames for r in g.frags[f]) and g.nrows % reps == 0
        self.nwin = g.nrows // reps
        coord = g.coord if g.strand > 0 else g.coord - (self.nwin + k - 1) + 1         # Seqinfo.start; end = start + len - 1
        self.record, self.names = fragment_cluster(k, self.nwin, frags, g.strand, coord, g.offset, seed=1000 * k + reps)
        self.stroi = {self.names[0]}
        self.texts = Texts(*oracle_texts([self.record], klength=k, canon=canon, stroi=self.stroi, maf=0.0))
        self.edges = list(g.edges) + ([f"key_width:k{k}:{'canon' if canon else 'both'}"] if geo == "two" else [])

    def hash_of(self, f):
        """the hash of the rows of fragment f (the claim that it is one hash, and the fragment's alone, is the CPU test's)"""
        return self.texts.row_hash[self.geo.frags[f][0]]

    def target_hash(self):
        inside = {r for a, b in self.geo.frags.values() for r in range(a, b)}
        return self.texts.row_hash[next(r for r in range(self.geo.nrows) if r not in inside)]

    def passing(self, lst):
        what = self.geo.lists[lst][0]
        return list(self.texts.hashes) if what == ALL else [self.target_hash()] if what == TARGET else [self.hash_of(f) for f in what]

    def claim(self, lst):
        """the row indices the list is built to keep"""
        what = self.geo.lists[lst][0]
        inside = sorted({r for a, b in self.geo.frags.values() for r in range(a, b)})
        if what == ALL:
            return list(range(self.geo.nrows))
        if what == TARGET:
            return [r for r in range(self.geo.nrows) if r not in set(inside)]
        return sorted(r for f in what for r in range(*self.geo.frags[f]))

    def units(self, lst):
        return tile_units(self.texts.rows, self.texts.kept(self.passing(lst)), {seq_key(self.texts.rows[0]): self.geo.nrows})


@functools.lru_cache(maxsize=None)
def fragment_case(geo, k, canon):
    return FragmentCase(geo, k, canon)


# ----------------------------------------------------------------------------------------------- 2. several arenas
ARENA_K = 31


@functools.lru_cache(maxsize=None)
def arena_batch():
    """(records, target strains, Texts, the middle cluster's name): a small cluster, the cluster that overflows its scan
    table twice (kmer_content.back_loaded_cluster), a small cluster; two targets in each"""
    mid, names = kc.back_loaded_cluster(16, 36, 1500, head=500, seed=5)
    rng = np.random.default_rng(52)

    def nested(n, length):
        """allele j carries the first j of n - 1 substitutions: the windows over substitution i are shared by the alleles
        from i on, or by those before it -- several patterns along every sequence"""
        anc = bytearray(kc.rand_seq(rng, length))
        out = [bytes(anc)]
        for j in range(1, n):
            p = 40 + 57 * j
            anc[p] = ord("ACGT"[("ACGT".index(chr(anc[p])) + 1) % 4])
            out.append(bytes(anc))
        return out
    small = [kc.cluster(f"g_small{i}", names, [(f"s{i}_{j}", a) for j, a in enumerate(nested(5, 340 + 23 * i))]) for i in range(2)]
    recs = [small[0], mid, small[1]]
    stroi = {names[1], names[18]}                # a tandem repeat's carrier and a late unique allele's
    t = Texts(*oracle_texts(recs, klength=ARENA_K, stroi=stroi, maf=0.0))
    return recs, stroi, t, mid[1]


# ----------------------------------------------------------------------------------------------- 3. batches, growing table
GROW_UP, GROW_DOWN, GROW_K, GROW_BATCH = 40, 30, 21, 4
# clusters, strains, first seed, mean alleles -> rows, rows listed, patterns (> the 512 of a 1 024-slot table's pool),
# rows kept by every second hash
GROW_TABLE = dict(clusters=20, strains=64, seed=2121, mean_alleles=10.0, rows=94095, listed=94095, patterns=1798, kept=47615)
GrowCase = collections.namedtuple("GrowCase", "csvp gffdir targets texts by_cluster n_patterns")


@functools.lru_cache(maxsize=None)
def grow_case():
    """passing_cases.case's kind of pangenome with more strains and alleles, written to disk for run_pangenome"""
    import atexit
    import shutil
    import tempfile

    from oracle import input_restatement as ir
    from oracle import oracle as po
    from panfeed_amd import synth
    g = GROW_TABLE
    root = tempfile.mkdtemp(prefix="passing_grow_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    cl = synth.generate(g["clusters"], g["strains"], first=g["seed"], flank=0, mean_len=250, min_len=80, max_len=700,
                        n_rate=0.2, paralog_rate=0.05, mean_alleles=g["mean_alleles"])
    names = cl[0].names
    csvp, gffs, _fas = synth.write_pangenome(root, cl)
    targets = tuple(names[i] for i in range(0, g["strains"], 4))
    strains, table = ir.load_table(csvp)
    gn = sorted(gffs)
    recs = list(ir.iter_gene_clusters(strains, table, ir.load_genomes(gn, [gffs[n] for n in gn]), GROW_UP, GROW_DOWN, False))
    run = po.OracleRun(klength=GROW_K, stroi=set(targets), canon=True, maf=0.0)
    run.feed(recs)
    t = Texts(*run.texts())
    by_cluster = collections.OrderedDict((r[1], []) for r in recs)
    for i, r in enumerate(t.rows):
        by_cluster[r.split("\t", 1)[0]].append(i)
    return GrowCase(csvp, root + "/gffs", targets, t, by_cluster, t.hp.count("\n"))


def grow_passing(c):
    return c.texts.hashes[::2]


# ----------------------------------------------------------------------------------------------- 4. chains that wrap
def mix64(x):
    """pass_mix64"""
    x &= MASK64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK64
    return x ^ (x >> 31)


def digest_words(h):
    """(d0, d1) of a 24-character hash as the library reads its 16 bytes"""
    d = base64.b64decode(h)
    return int.from_bytes(d[:8], "little"), int.from_bytes(d[8:], "little")


def digest_hash(h):
    """pass_digest_hash at 64 bits"""
    d0, d1 = digest_words(h)
    return mix64(d0 ^ mix64(d1))


def key_words_of(kmer):
    """the arena's key of a k-mer (the comment above kt_row_passes): the 2k-bit value, first base most significant, in
    63-bit words, the most significant first"""
    k = len(kmer)
    v = 0
    for ch in kmer:
        v = (v << 2) | kc._CODE[ch]
    KW = kc.key_words(k)
    return [(v >> (63 * (KW - 1 - w))) & ((1 << 63) - 1) for w in range(KW)]


def key_hash(cluster, kmer):
    """pass_key_hash at 64 bits"""
    h = mix64(cluster + 0x9e3779b97f4a7c15)
    for w in key_words_of(kmer):
        h = mix64(h ^ w)
    return h


def occupied(homes, cap):
    """the slots a linear-probing table of `cap` holds after these homes went in -- whatever their order"""
    used = [False] * cap
    for h in homes:
        while used[h]:
            h = (h + 1) & (cap - 1)
        used[h] = True
    return used


def wraps(homes, cap):
    """the order-independent condition: a t with more than t entries homed in the top t slots"""
    return any(sum(1 for h in homes if h >= cap - t) > t for t in range(1, cap))


def probe_wraps(home, used):
    """a probe from `home` finds every slot up to the table's last one taken"""
    return all(used[home:])


WRAP_K, WRAP_NWIN, WRAP_CAP = 31, 511, 1024
WRAP_FRAGS = [(16 * j + 3, 16 * j + 5) for j in range(31)]
WRAP_SEED = 1                   # set by _find_wrap_seed; the GPU test holds it against the device's own table


class WrapIndex:
    """a fragment cluster of 511 kept k-mers (an index of 1 024 slots, half full) whose chains wrap, and a fragment whose
    k-mers, left out, send a probe round the table's end to a free slot"""

    def __init__(self, seed=WRAP_SEED):
        self.k = WRAP_K
        self.record, self.names = fragment_cluster(WRAP_K, WRAP_NWIN, WRAP_FRAGS, seed=seed)
        self.stroi = {self.names[0]}
        self.texts = t = Texts(*oracle_texts([self.record], klength=WRAP_K, stroi=self.stroi, maf=0.0))
        self.kmers = [r.rsplit("\t", 1)[1] for r in t.rows]                 # row i prints the key of place i
        self.homes = [key_hash(0, km) & (WRAP_CAP - 1) for km in self.kmers]

    def without(self, j):
        """(the list without fragment j's hash, the places of its rows)"""
        a, b = WRAP_FRAGS[j]
        h = self.texts.row_hash[a]
        return [x for x in self.texts.hashes if x != h], list(range(a, b))

    def absent_wrapping(self):
        """fragments whose removal leaves a wrapped run that a probe for one of their keys has to cross"""
        out = []
        for j in range(len(WRAP_FRAGS)):
            _, places = self.without(j)
            used = occupied([h for i, h in enumerate(self.homes) if i not in places], WRAP_CAP)
            if any(probe_wraps(self.homes[i], used) for i in places):
                out.append(j)
        return out


@functools.lru_cache(maxsize=None)
def wrap_index():
    return WrapIndex()


def _find_wrap_seed(limit=200):
    """how WRAP_SEED was found: the first seed whose index wraps and has a fragment for the absent case"""
    for seed in range(limit):
        w = WrapIndex(seed)
        if wraps(w.homes, WRAP_CAP) and w.absent_wrapping():
            return seed, w.absent_wrapping()
    return None


SET_CAP, SET_FILLERS = 64, 22


class WrapSet:
    """a passing list of 1 + 22 digests in a set of 64 slots: the hash `present` (rows have it), 22 fillers no row has,
    homed so that the chain of `present` and the probe for `absent` (a hash of the cluster left out of the list) cross
    the table's end"""

    def __init__(self, w):
        import hashlib
        t = w.texts
        homes = {h: digest_hash(h) & (SET_CAP - 1) for h in t.hashes}
        # the two real hashes homed highest: the fewer slots behind them, the sooner the run is full
        self.present, self.absent = sorted(t.hashes, key=lambda h: -homes[h])[:2]
        lo = min(homes[self.present], homes[self.absent])
        self.fillers, i = [], 0
        while len(self.fillers) < SET_FILLERS:
            h = base64.b64encode(hashlib.md5(b"filler %d" % i).digest()).decode()
            i += 1
            if h not in t.pairs.values() and digest_hash(h) & (SET_CAP - 1) >= lo:
                self.fillers.append(h)
        self.lo = lo
        self.list = [self.present] + self.fillers

    def homes(self, hashes):
        return [digest_hash(h) & (SET_CAP - 1) for h in hashes]


@functools.lru_cache(maxsize=None)
def wrap_set():
    return WrapSet(wrap_index())


# ----------------------------------------------------------------------------------------------- 5. content
CONTENT_CASES = [(32, True), (64, True), (126, True), (32, False), (64, False)]


class ContentCase:
    def __init__(self, k, canon):
        self.k, self.canon = k, canon
        self.recs, self.names, self.kinds = kc.content_clusters(k)
        self.stroi = set(self.names)
        self.texts = t = Texts(*oracle_texts(self.recs, klength=k, canon=canon, stroi=self.stroi, maf=0.0))
        self.models = kc.model_clusters(self.recs, k, canon, self.stroi)
        # every second distinct hash in file order.  A sequence and its reverse complement share every k-mer, so their
        # rows have one hash between them (that of their carriers' union); on this content it is an odd one of the
        # file, and the list shifted by one drops the homopolymer's instead: the list is every second hash plus that one
        self.passing = t.hashes[0::2]
        self.added = []
        if "fwd_rc" in content_conditions(self, self.passing):
            fwd = self.kinds[0]["fwd"]
            self.added = [next(h for r, h in zip(t.rows, t.row_hash) if r.split("\t", 2)[:2] == ["g_pal", fwd] and h)]
            self.passing = self.passing + self.added


def content_conditions(c, passing):
    """what the list must do on this content; returns the conditions it misses"""
    t, k = c.texts, c.k
    keep = set(t.kept(passing))
    missed = []

    def split(name, rows):
        if not (any(i in keep for i in rows) and any(i not in keep for i in rows)):
            missed.append(name)
    kmer = [r.rsplit("\t", 1)[1] for r in t.rows]
    rcs = [kc.rc(km.encode()).decode() for km in kmer]
    split("palindrome", [i for i, km in enumerate(kmer) if km == rcs[i]])
    second = []
    for i, km in enumerate(kmer):
        cls = kc.classify(km, rcs[i], k)
        if cls is not None and cls[0] >= 1:
            second.append(i)
    split("second_word", second)
    if not c.canon:
        at = {("AT" * k)[:k], ("TA" * k)[:k]}
        pairs = [(i, i + 1) for i in range(0, len(kmer) - 1) if kmer[i] in at and kmer[i + 1] == kmer[i] and
                 t.rows[i].rsplit("\t", 2)[0] == t.rows[i + 1].rsplit("\t", 2)[0]]
        both = [(a in keep, b in keep) for a, b in pairs]
        if not pairs or (True, True) not in both or (False, False) not in both or any(a != b for a, b in both):
            missed.append("at_pairs")
    for kind in ("fwd", "rc"):
        strain = c.kinds[0][kind]
        if not any(i in keep for i, r in enumerate(t.rows) if r.split("\t", 2)[:2] == ["g_pal", strain]):
            missed.append("fwd_rc")
    seqs = collections.OrderedDict()
    for i, r in enumerate(t.rows):
        seqs.setdefault(seq_key(r), []).append(i)
    rep_a = [rows for rows in seqs.values() if kmer[rows[0]] in ("A" * k, "T" * k) and len(set(kmer[i] for i in rows)) <= 2]
    if not any(all(i in keep for i in rows[:KT_ROWS]) for rows in rep_a):
        missed.append("rep_A_tile")
    return missed


@functools.lru_cache(maxsize=None)
def content_case(k, canon):
    return ContentCase(k, canon)


# ----------------------------------------------------------------------------------------------- who claims which edge
def claims():
    """(case, the edges it stands on) of every case above; test_passing_edges.py checks each and holds the union
    against EDGES"""
    out = []
    for geo, k, canon in FRAGMENT_CASES:
        c = fragment_case(geo, k, canon)
        out.append((c.name, c.edges + [e for _, edges in c.geo.lists.values() for e in edges]))
    out.append(("arena_batch", ["arenas:retried_between_two_small"]))
    out.append(("grow_case", ["batches:pattern_table_grows", "batches:pattern_of_batch_1_in_a_later_batch"]))
    out.append(("wrap_index", ["wrap:index_present", "wrap:index_absent"]))
    out.append(("wrap_set", ["wrap:set_present", "wrap:set_absent", "set:fillers_only"]))
    for k, canon in CONTENT_CASES:
        m = "canon" if canon else "both"
        out.append((f"content-k{k}-{m}", [f"content:{c}:{m}" for c in ("palindrome", "second_word", "fwd_rc", "rep_A_tile")] +
                    ([] if canon else ["content:at_pairs:both"])))
    return out
