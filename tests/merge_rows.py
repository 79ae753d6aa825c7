"""Rows for the pattern merge table and what must come out of it.  numpy and dict only: no library, no torch.

After the ranks of a sharded run exchange {md5 lo, md5 hi, first_seen}, pf_merge_patterns / pf_merge_patterns_padded mark one
row per digest, the one with the smallest first_seen (merge_slot, merge_insert_kernel, merge_lookup_kernel in
panfeed_amd/csrc/pf_kernels.h, driven by merge_impl in pf_api.hip).  marks() below is that rule with a Python dict in the
table's place.  The case builders make the rows real MD5 digests never give: equal first or second words, probe chains that
run over the end of the table, the words next to the table's empty marker, a wave whose lanes all carry one digest, and
padding that looks like real rows.  tests/test_merge_rows.py holds the model against the torch sort and checks that every
case reaches what it claims; tests/test_gpu_merge_table.py holds the kernels against the model.

Two limits of the kernels are part of the model, and every case stays inside them:

* first_seen < 2^63.  The device orders first_seen as unsigned (atomicMin on unsigned long long), the torch route of
  distributed._first_per_digest orders int64, and the two agree only below 2^63.  A run's values lie there: cluster
  ordinal << 32 | rank inside the cluster.
* all-ones aliasing.  The table's empty marker is the all-ones word, so merge_slot maps a digest word equal to it to
  all-ones - 1 before it hashes or compares.  The digests (all-ones, h) and (all-ones - 1, h) are therefore ONE digest to
  the kernels, and likewise in the second word: a known limit, 2^-64 per pair of MD5 digests.  marks() groups by the words
  as they are and does NOT alias; aliased() says whether a set of rows holds such a pair, and no case does.
"""
import itertools

import numpy as np

ONES = 0xFFFFFFFFFFFFFFFF             # EMPTY64 of pf_kernels.h: the table's empty marker
FS_LIMIT = 1 << 63
MIN_SLOTS = 1024
WAVE = 64
_U = np.uint64


def marks(rows, counts=None, slot_rows=0):
    """rows: uint64 [n,3] = {digest lo, digest hi, first_seen}.  (keep bool [n], n_distinct): keep[i] is true where
    first_seen equals the minimum of the rows with that (lo, hi), so a tie marks both rows.  With counts and slot_rows the
    rows come in slots of slot_rows per rank and only the first counts[r] rows of slot r exist: the others neither join a
    group nor get marked."""
    rows = np.asarray(rows, dtype=_U).reshape(-1, 3)
    live = existing(rows.shape[0], counts, slot_rows)
    least = {}
    for i in np.flatnonzero(live):
        d, fs = (int(rows[i, 0]), int(rows[i, 1])), int(rows[i, 2])
        if d not in least or fs < least[d]:
            least[d] = fs
    keep = np.zeros(rows.shape[0], dtype=bool)
    for i in np.flatnonzero(live):
        keep[i] = int(rows[i, 2]) == least[(int(rows[i, 0]), int(rows[i, 1]))]
    return keep, len(least)


def existing(n, counts=None, slot_rows=0):
    """bool [n]: the rows that are not padding"""
    if counts is None or not slot_rows:
        return np.ones(n, dtype=bool)
    assert n == len(counts) * slot_rows and all(0 <= c <= slot_rows for c in counts)
    return (np.arange(slot_rows)[None, :] < np.asarray(counts)[:, None]).reshape(-1)


# --- the table's geometry, restated here as an ASSUMPTION the `wrap` case is built on (taken from merge_impl in
# --- csrc/pf_api.hip: the capacity; and merge_slot in csrc/pf_kernels.h: the remap and the home slot).  If the library
# --- changes either, `wrap` still checks the marks but may no longer run over the table's end.
def capacity(n):
    cap = MIN_SLOTS
    while cap < 2 * n:
        cap <<= 1
    return cap


def table_key(lo, hi):
    """the words as the table stores them: the empty marker is kept out of the key space"""
    return (ONES - 1 if lo == ONES else lo, ONES - 1 if hi == ONES else hi)


def home_slot(lo, hi, cap):
    lo, hi = table_key(lo, hi)
    return (lo ^ (hi >> 17)) & (cap - 1)


def occupied_slots(rows):
    """the slots the rows' digests take under linear probing from home_slot (the set does not depend on the order of
    insertion), and the table's size"""
    cap = capacity(len(rows))
    taken = set()
    for lo, hi in sorted({table_key(int(r[0]), int(r[1])) for r in rows}):
        s = home_slot(lo, hi, cap)
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
    return taken, cap


def aliased(rows):
    """true if two different digests among the rows are one digest to the kernels (see the module docstring)"""
    raw = {(int(r[0]), int(r[1])) for r in rows}
    return len({table_key(*d) for d in raw}) != len(raw)


def ranges(n):
    """(first, count) of the rows a rank asks marks for: everything, each third, one row at either end, and nothing"""
    a, b = n // 3, 2 * n // 3
    out = [(0, n), (0, a), (a, b - a), (b, n - b), (0, 1), (n - 1, 1), (0, 0)]
    return list(dict.fromkeys(out))


# --- builders -------------------------------------------------------------------------------------------------
def _words(rng, n):
    """n distinct random words, none of them 0 or next to the empty marker"""
    w = rng.integers(1, ONES - 1, size=n, dtype=_U)
    assert len(set(w.tolist())) == n
    return w


def _first_seens(rng, n):
    """n distinct values shaped like a run's: cluster ordinal << 32 | rank inside the cluster, in random order"""
    ordinal = rng.permutation(n).astype(_U) + _U(1)
    return (ordinal << _U(32)) | rng.integers(0, 1 << 16, size=n, dtype=_U)


def _rows(lo, hi, fs):
    out = np.empty((len(lo), 3), dtype=_U)
    out[:, 0], out[:, 1], out[:, 2] = lo, hi, fs
    return out


def _copies(rng, digests, copies):
    """digest d `copies[d]` times, the rows shuffled, with distinct first_seen"""
    idx = rng.permutation(np.repeat(np.arange(len(digests)), copies))
    return _rows(digests[idx, 0], digests[idx, 1], _first_seens(rng, len(idx)))


def _same_word(col, seed, extra):
    """512 digests that share word `col`; `extra` of them come a second time and half as many of those a third time"""
    rng = np.random.default_rng(seed)
    d = np.empty((512, 2), dtype=_U)
    d[:, col] = _words(rng, 1)[0]
    d[:, 1 - col] = _words(rng, 512)
    copies = np.ones(512, dtype=np.int64)
    pick = rng.permutation(512)
    copies[pick[:extra]] += 1
    copies[pick[:extra // 2]] += 1
    return _copies(rng, d, copies)


def _wrap():
    rng = np.random.default_rng(31)
    hi = _words(rng, 40)
    want = _U(MIN_SLOTS - 8) + (np.arange(40, dtype=_U) % _U(8))                    # the last 8 slots, 5 digests each
    lo = (_words(rng, 40) & ~_U(MIN_SLOTS - 1)) | ((want ^ (hi >> _U(17))) & _U(MIN_SLOTS - 1))
    return _copies(rng, np.stack([lo, hi], axis=1), np.full(40, 2))


def _three_copies(digests, seed):
    """every digest three times; which copy (in row order) holds the smallest first_seen goes through all six orders"""
    rng = np.random.default_rng(seed)
    nd = len(digests)
    orders = list(itertools.permutations(range(3)))
    base = np.sort(_first_seens(rng, 3 * nd)).reshape(nd, 3)                         # digest i: base[i,0] < [i,1] < [i,2]
    lo, hi, fs = [], [], []
    for copy in range(3):                                                         # copy-major: a digest's rows lie nd apart
        for i, (a, b) in enumerate(digests):
            lo.append(a), hi.append(b), fs.append(base[i, orders[i % 6][copy]])
    return _rows(lo, hi, fs)


def _sentinel_lo():
    h = [int(x) for x in _words(np.random.default_rng(41), 8)]
    return _three_copies([(ONES, h[0]), (ONES - 1, h[1]), (0, h[2]), (h[3], 0), (0, 0), (ONES, 0), (ONES - 1, h[4]),
                          (ONES, h[5]), (1, h[6]), (ONES - 2, h[7])], 42)


def _sentinel_hi():
    w = [int(x) for x in _words(np.random.default_rng(43), 8)]
    return _three_copies([(w[0], ONES), (w[1], ONES - 1), (0, ONES), (w[2], ONES), (w[3], ONES - 1), (ONES, ONES),
                          (ONES - 1, w[4]), (w[5], ONES - 2), (w[6], 1), (1, ONES - 1)], 44)


def _one_digest(where):
    rng = np.random.default_rng(51)
    lo, hi = (int(x) for x in _words(rng, 2))
    fs = _first_seens(rng, 4096)
    m = int(np.argmin(fs))
    fs[m], fs[where] = fs[where], fs[m]
    return _rows(np.full(4096, lo, dtype=_U), np.full(4096, hi, dtype=_U), fs)


def _wave_shapes(lanes_equal):
    rng = np.random.default_rng(61)
    d = np.stack([_words(rng, WAVE), _words(rng, WAVE)], axis=1)
    i = np.arange(WAVE * WAVE)
    which = i // WAVE if lanes_equal else i % WAVE
    return _rows(d[which, 0], d[which, 1], _first_seens(rng, len(i)))


def _ties_and_zero():
    w = [int(x) for x in _words(np.random.default_rng(71), 12)]
    top = FS_LIMIT - 1
    return _rows(*zip(
        (w[0], w[1], 7 << 32), (w[2], w[3], 0), (w[4], w[5], top), (w[0], w[1], 7 << 32),      # a tie; 0 alone; 2^63-1 alone
        (w[6], w[7], top), (w[6], w[7], 0), (w[6], w[7], 1),                                  # 0 beats 1 beats 2^63-1
        (w[8], w[9], 5), (w[8], w[9], 9), (w[8], w[9], 5), (w[8], w[9], 5),                   # a three-way tie below a loser
        (w[10], w[11], top), (w[10], w[11], top)))                                            # a tie at the largest value


def _sizes(n):
    rng = np.random.default_rng(80 + n)
    return _rows(_words(rng, n), _words(rng, n), _first_seens(rng, n))


def unpadded_cases():
    """name -> (rows uint64 [n,3], [(my_first, my_count)])"""
    made = {
        "same_lo/536": _same_word(0, 11, 16),                  # 512 + 16 + 8 = 536 rows: 2 048 slots
        "same_hi/536": _same_word(1, 12, 16),
        "wrap": _wrap(),
        "sentinel_lo": _sentinel_lo(),
        "sentinel_hi": _sentinel_hi(),
        "one_digest/min_first": _one_digest(0),
        "one_digest/min_last": _one_digest(4095),
        "one_digest/min_middle": _one_digest(2048),
        "wave_shapes/lanes_equal": _wave_shapes(True),
        "wave_shapes/lanes_differ": _wave_shapes(False),
        "ties_and_zero": _ties_and_zero(),
    }
    for word in ("same_lo", "same_hi"):                        # the same digests once each: 512 rows fill half of 1 024 slots
        full = made[word + "/536"]
        _, first = np.unique(full[:, :2], axis=0, return_index=True)
        made[word + "/512"] = full[np.sort(first)]
    for n in (1, 2, 511, 512, 513, 1024, 1025):
        made[f"sizes/{n}"] = _sizes(n)
    return {name: (rows, ranges(len(rows))) for name, rows in made.items()}


PAD_WORLD, PAD_SLOT_ROWS = 4, 300
PAD_COUNTS = (PAD_SLOT_ROWS, 0, 1, PAD_SLOT_ROWS - 1)
PADDINGS = ("early_copies", "all_ones", "fresh")


def padded_cases():
    """name -> (rows uint64 [world * slot_rows, 3], counts, slot_rows): one set of real rows (rank 3 and rank 2 saw half of
    rank 0's digests again, some earlier, some later) in front of three kinds of padding"""
    rng = np.random.default_rng(91)
    S = PAD_SLOT_ROWS
    d0 = np.stack([_words(rng, S), _words(rng, S)], axis=1)
    fs = _first_seens(rng, 2 * S) + (_U(1) << _U(48))            # room below for padding that claims to be earlier
    again = rng.permutation(S)[: S // 2]
    d3 = np.stack([_words(rng, S - 1), _words(rng, S - 1)], axis=1)
    d3[: S // 2] = d0[again]
    d3 = d3[rng.permutation(S - 1)]
    real = {0: _rows(d0[:, 0], d0[:, 1], fs[:S]), 2: _rows(d0[again[:1], 0], d0[again[:1], 1], fs[S:S + 1]),
            3: _rows(d3[:, 0], d3[:, 1], fs[S + 1:])}
    every = np.concatenate([real[0], real[2], real[3]])
    out = {}
    for kind in PADDINGS:
        n = PAD_WORLD * S
        if kind == "early_copies":
            src = every[rng.integers(0, len(every), size=n)]
            rows = _rows(src[:, 0], src[:, 1], np.arange(n, dtype=_U))              # all below 2^48 <= every real first_seen
        elif kind == "all_ones":
            rows = np.full((n, 3), ONES, dtype=_U)
        else:
            rows = _rows(_words(rng, n), _words(rng, n), _first_seens(rng, n))
        for r, x in real.items():
            assert len(x) == PAD_COUNTS[r]
            rows[r * S:r * S + len(x)] = x
        out[f"padded/{kind}"] = (rows, PAD_COUNTS, S)
    return out
