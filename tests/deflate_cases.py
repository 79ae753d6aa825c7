"""Inputs of the device gzip tests (tests/test_deflate_host_model.py on the CPU, tests/test_gpu_deflate.py on the GPU): the
smallest texts at which a chunked one-candidate LZ77 + Huffman coder can go wrong.  `cases(C)` yields
(name, data, flag sets); C is pf_gzip_device_chunk_bytes()."""
import functools
import gzip
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_tokens as dt  # noqa: E402

FIXED_ONLY, DYNAMIC_ONLY, LITERALS_ONLY = 1, 2, 4
FIXED, DYNAMIC = dt.FIXED, dt.DYNAMIC
ALL = (0, FIXED_ONLY, DYNAMIC_ONLY)

# the first and the last length of each of the length symbols 258..285 (symbol 257, length 3, cannot be emitted: see
# match_ok in csrc/pf_deflate.h)
LENGTH_EDGES = tuple(sorted({L for sym in range(258, 286) for L in dt.length_range(sym)}))
# the first distance of each of the distance symbols 0..29
DISTANCE_EDGES = dt.DIST_BASE[:26]
FAR_DISTANCE_EDGES = dt.DIST_BASE[26:] + (32768,)
RUN_LENGTHS = (1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 516, 517)


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


class _Cells:
    """a text under construction: position i holds the byte of variable ids[i]; a copy shares its source's variables,
    so a byte drawn again changes every place it stands in"""

    def __init__(self, seed):
        self.rng, self.ids, self.vals, self.fixed = random.Random(seed), [], [], set()

    def fresh(self, n):
        at = len(self.ids)
        self.ids += range(len(self.vals), len(self.vals) + n)
        self.vals += self.rng.randbytes(n)
        return at

    def put(self, value):
        """a byte that is never drawn again"""
        self.fixed.add(len(self.vals))
        self.ids.append(len(self.vals))
        self.vals.append(value)

    def copy(self, src, n):
        at = len(self.ids)
        self.ids += self.ids[src:src + n]
        return at

    def text(self):
        return bytes(self.vals[v] for v in self.ids)

    def clear_buckets(self, pairs):
        """draw bytes again until, for every (S, P) of `pairs`, no position between S and P has the hash4 of position
        S: the one-entry bucket of S still names S when the encoder reaches P, under either match rule"""
        for _ in range(200):
            text = self.text()
            h = dt.hashes(text)
            where = {}
            for q, x in enumerate(h):
                where.setdefault(x, []).append(q)
            redraw = set()
            for S, P in pairs:
                keep = set(self.ids[S:S + 4]) | self.fixed
                for q in where[h[S]]:
                    if S < q < P:
                        # (a position made of the source's own and of fixed bytes: the source is drawn again)
                        free = [v for v in self.ids[q:q + 4] if v not in keep] or [self.ids[S + 3]]
                        redraw.add(free[-1])
            if not redraw:
                return text
            for v in sorted(redraw):
                self.vals[v] = self.rng.randrange(256)
        raise AssertionError("the buckets did not come clear")


@functools.lru_cache(maxsize=None)
def length_edge(L):
    """300 random bytes R, a byte absent from R, R[:L], then a byte different from R[L]: one match, (L, 301).  R is drawn
    until no position 1..300 falls into the hash bucket of position 0, which the match's candidate comes from."""
    for seed in range(1000 * L, 1000 * L + 1000):
        R = _rand(seed, 300)
        absent = [b for b in range(256) if b not in R]
        if not absent:
            continue
        text = R + bytes([absent[0]]) + R[:L] + bytes([(R[L] + 1) & 0xFF])
        h = dt.hashes(text)
        if h[0] not in h[1:301]:
            return text
    raise AssertionError(f"no text for length {L}")


@functools.lru_cache(maxsize=None)
def distance_edge(D):
    """D >= 8: an 8-byte block, random filler, the block again exactly D bytes after its first occurrence, the filler
    drawn until no position between the two falls into the block's hash bucket: the text ends with the match (8, D).
    D < 8: 40 bytes of period D, which end with a match at distance D (from position D under the host model's rule,
    from position 8, the first with a group of eight before it, under the kernel's)."""
    for seed in range(2000 * D, 2000 * D + 1000):
        cells = _Cells(seed)
        if D < 8:
            cells.fresh(D)
            while len(cells.ids) < 40:
                cells.copy(len(cells.ids) - D, 1)
            text = cells.text()
            if len(set(dt.hashes(text)[:D])) == D:
                return text
            continue
        cells.fresh(D)
        cells.copy(0, 8)
        try:
            return cells.clear_buckets([(0, D)])
        except AssertionError:
            continue
    raise AssertionError(f"no text for distance {D}")


def _fib():
    F = [0, 1, 1]
    while len(F) < 64:
        F.append(F[-1] + F[-2])
    return F


@functools.lru_cache(maxsize=None)
def fibonacci_counts(C):
    """byte value i occurs F(i) times, i = 2..m, m the largest with F(m + 2) - 2 <= C.  With the end-of-block symbol,
    which occurs once, the frequencies are F(1), F(2), .. F(m): the one chain a Huffman tree of Fibonacci weights is,
    m - 1 >= 17 bits deep unlimited."""
    F = _fib()
    m = max(i for i in range(2, 40) if F[i + 2] - 2 <= C)
    assert m >= 18
    data = bytearray()
    for i in range(2, m + 1):
        data += bytes([i]) * F[i]
    random.Random(7).shuffle(data)
    return bytes(data)


# four of each length symbol with 5 extra bits, 281..284
WIDE_LENGTHS = (140, 170, 200, 235, 145, 175, 205, 240, 150, 180, 210, 245, 155, 185, 215, 250)
# near matches: one distance of each distance symbol 5..12 and how many of it at 32 KiB, each count about the sum of
# those behind it and of the far symbols' 8 + 8: the distance code is a chain as deep as it has symbols
NEAR_MATCHES = ((8, 960), (9, 480), (13, 240), (17, 120), (25, 60), (33, 30), (49, 15), (65, 16))


@functools.lru_cache(maxsize=None)
def wide_tokens(C, seed=15):
    """One chunk whose dynamic block holds tokens of about 40 bits, of which put_bits writes some into three words.
    A token is widest with a length symbol of 5 extra bits and a distance symbol of the most extra bits a chunk allows
    (13 at 32 KiB), both rare and so deep in their codes: sixteen long blocks come back once each at the end, half a
    chunk or more later, while in between mostly random literals fill the literal / length code and near matches
    (chains of a 4-byte block, filler, the block again) fill the distance code.  Every match's source stands 8 bytes or
    more before its copy, and between the two nothing falls into its hash bucket: both match rules give the same tokens.
    (The seed is the one of 11..18 at which most tokens, 8 of the 16 wide ones, reach a third word at 32 KiB; each of
    those seeds gives at least one.)"""
    cells = _Cells(seed)
    pairs, far = [], []

    def sources(lengths):
        for L in lengths:
            far.append((cells.fresh(L), L))
            cells.fresh(9)

    tail = sum(L + 9 for L in WIDE_LENGTHS)
    sources(WIDE_LENGTHS[:8])                               # these end up 24 577 or more before their copies at 32 KiB
    for d, count in NEAR_MATCHES:
        if len(far) == 8 and len(cells.ids) >= 3 * C // 10:
            sources(WIDE_LENGTHS[8:])                       # and these between 16 385 and 24 576
        for i in range(max(1, count * C // 32768)):
            if i % 192 == 0:                                # a new chain, of another block
                cells.fresh(9)
                S = cells.fresh(4)
            cells.fresh(d - 5)
            cells.put(i % 192)                              # the byte before each copy differs along the chain: no
            P = cells.copy(S, 4)                            # copy is matched from one byte early against an older one
            pairs.append((S, P))
            S = P
        cells.fresh(9)
    if len(far) == 8:
        sources(WIDE_LENGTHS[8:])
    cells.fresh(C - 64 - tail - len(cells.ids))
    for S, L in far:
        pairs.append((S, cells.copy(S, L)))
        cells.fresh(9)
    assert len(cells.ids) <= C
    return cells.clear_buckets(pairs)


@functools.lru_cache(maxsize=None)
def every_length_symbol():
    """the texts of the first length of each length symbol 258..285, between them a byte that is not the next text's
    absent one: every symbol in one chunk"""
    out = b""
    for sym in range(258, 286):
        piece = length_edge(dt.length_range(sym)[0])
        out += (b"\n" if piece[300] != 10 else b"\t") + piece
    return out


@functools.lru_cache(maxsize=None)
def fixed_chunk(C):
    """a whole chunk for which the fixed codes are the smallest: random blocks of 8 to 65 bytes, each repeated over an
    eighth of the chunk -- some 350 tokens over many symbols, too few to pay for a dynamic block's header"""
    rng, periods = random.Random(1), (8, 9, 13, 17, 25, 33, 49, 65)
    seg = C // len(periods)
    return b"".join((rng.randbytes(p) * seg)[:seg] for p in periods) + b"\n" * (C - seg * len(periods))


def chunk_kinds(C):
    """whole chunks of six kinds, (name, text, block type or None: either rule's tokens are within a few bytes of a
    tie): what a workgroup meets one after the other in a long text"""
    def whole(text):
        return (text + _rand(9, C))[:C]
    return [("random", _rand(4, C), dt.STORED), ("rows", real_shapes(C)["hashes_to_patterns"][:C], dt.DYNAMIC),
            ("run", b"a" * C, None), ("wide_tokens", whole(wide_tokens(C)), dt.DYNAMIC),
            ("fibonacci", whole(fibonacci_counts(C)), dt.DYNAMIC), ("periods", fixed_chunk(C), dt.FIXED)]


@functools.lru_cache(maxsize=None)
def real_shapes(C):
    """about 5 C bytes of each of the three files' text: kmers_to_hashes rows, hashes_to_patterns rows at 100 strains
    with NaN cells, kmers.tsv rows -- from a small synthetic pangenome through the CPU oracle"""
    from oracle import oracle as po
    from panfeed_amd import synth
    clusters = synth.generate(10, 100, first=4200, flank=10, mean_len=300, min_len=80, max_len=600, n_rate=0.02,
                              paralog_rate=0.05)
    names = clusters[0].names
    run = po.OracleRun(klength=21, stroi={names[1], names[5], names[50]}, canon=True, consider_missing=True,
                       patfilt=True, maf=0.01)
    run.feed([c.record() for c in clusters])
    kmers_tsv, kmers_to_hashes, hashes_to_patterns = (t.encode() for t in run.texts())
    assert b"\t\t" in hashes_to_patterns
    want = 5 * C
    return {name: (text * (want // len(text) + 1))[:want + 13]
            for name, text in (("kmers_to_hashes", kmers_to_hashes), ("hashes_to_patterns", hashes_to_patterns),
                               ("kmers_tsv", kmers_tsv))}


def cases(C):
    for n in (0, 1, 2, 3, 4):                                                   # 1
        yield f"short{n}", b"pqrs"[:n], ALL
    every = bytes(range(256))
    yield "all_bytes_twice", every + every, ALL                                 # 2
    for n in RUN_LENGTHS + (C - 1, C, C + 1, 2 * C + 3):                          # 3
        yield f"run{n}", b"a" * n, ALL
        yield f"period2_{n}", (b"0\t" * (n // 2 + 1))[:n], ALL
    for L in LENGTH_EDGES:                                                      # 4
        yield f"len{L}", length_edge(L), ALL
    for D in DISTANCE_EDGES + tuple(d for d in FAR_DISTANCE_EDGES if d + 8 <= C):   # 5
        yield f"dist{D}", distance_edge(D), ALL
    yield "incompressible", _rand(3, 3 * C + 17), (0,)                          # 6
    yield "fibonacci", fibonacci_counts(C), (LITERALS_ONLY | DYNAMIC_ONLY, DYNAMIC_ONLY)    # 7
    perm = bytearray(every)
    random.Random(8).shuffle(perm)
    yield "no_distance_symbol", bytes(perm), (DYNAMIC_ONLY,)                    # 8
    yield "one_literal_symbol", b"a" * 64, (LITERALS_ONLY | DYNAMIC_ONLY,)      # 9
    yield "wide_tokens", wide_tokens(C), (DYNAMIC_ONLY,)                        # 10
    yield "every_length_symbol", every_length_symbol(), ALL                     # 11
    for name, text in real_shapes(C).items():                                   # 12
        yield f"shape_{name}", text, ALL


def flat_cases(C):
    return [(f"{name}-f{flags}", data, flags) for name, data, flagset in cases(C) for flags in flagset]


def dump_cases(path, C):
    """wide_tokens and fibonacci under each of their flag sets as records of flags (u32), name length (u32), name, text
    length (u64), text, little-endian: what tools/deflate_host_check.cpp reads, having no Python to build them with"""
    with open(path, "wb") as fh:
        for name, data, flagset in (("wide_tokens", wide_tokens(C), (DYNAMIC_ONLY,)),
                                    ("fibonacci", fibonacci_counts(C), (LITERALS_ONLY | DYNAMIC_ONLY, DYNAMIC_ONLY))):
            for flags in flagset:
                fh.write(flags.to_bytes(4, "little") + len(name).to_bytes(4, "little") + name.encode())
                fh.write(len(data).to_bytes(8, "little") + data)


def check_members(data, members, C):
    """any gzip reader gets back the text: gzip.decompress walks all members and checks every CRC32 and ISIZE"""
    if not data:
        assert len(members) == 0
        return
    assert gzip.decompress(bytes(members)) == data


def incompressible_cap(n, C):
    return n + 32 * -(-n // C) + 32


# ---- what an encoder's members of a case must be, token by token: the same assertions for the host model (against
# dt.parse_host) and for the kernel (against dt.parse_device)
def chunks_of(data, C):
    return [data[at:at + C] for at in range(0, len(data), C)]


def _padded(used):
    """the symbols of an alphabet that carry a code: the used ones, and with fewer than two of them a second one"""
    if len(used) >= 2:
        return set(used)
    return set(used) | ({0, 1} if not used else {1 if used == {0} else 0})


def _audit_codes(m, what, bad):
    ll, d = dt.histograms(m.tokens)
    for kind, hist, lens in (("literal/length", ll, m.ll_len), ("distance", d, m.d_len)):
        used = {s for s, f in enumerate(hist) if f}
        coded = {s for s, n in enumerate(lens) if n}
        if dt.kraft(lens) != 1 << dt.MAX_BITS:
            bad.append(f"{what}: the {kind} code's Kraft sum is {dt.kraft(lens)} / {1 << dt.MAX_BITS}")
        if max(lens) > dt.MAX_BITS:
            bad.append(f"{what}: a {kind} code of {max(lens)} bits")
        if coded != _padded(used):
            bad.append(f"{what}: {kind} symbols with a code {sorted(coded ^ _padded(used))} differ from the used ones")
        cost, (best, depth) = sum(f * n for f, n in zip(hist, lens)), dt.huffman(hist)
        if depth <= dt.MAX_BITS and cost != best:
            bad.append(f"{what}: the {kind} code costs {cost} bits, Huffman's {best}")
        if depth > dt.MAX_BITS and (max(lens) != dt.MAX_BITS or cost < best):
            bad.append(f"{what}: the limited {kind} code is {max(lens)} bits deep and costs {cost}, Huffman's {best}")


def audit(name, data, flagset, encode, parse, C):
    """encode(data, flags) -> members, for every flag set of the case; parse: the encoder's match rule.  Returns the
    failures, as strings, and {flags: decoded members}."""
    bad, decoded = [], {}
    chunks = chunks_of(data, C)
    for flags in flagset:
        what = f"{name}-f{flags}"
        try:
            ms = dt.members(encode(data, flags))
        except dt.BadStream as e:
            bad.append(f"{what}: {e}")
            continue
        if [m.text for m in ms] != chunks:
            bad.append(f"{what}: the members' texts are not the text's chunks")
            continue
        decoded[flags] = ms
        forced = FIXED if flags & FIXED_ONLY else DYNAMIC if flags & DYNAMIC_ONLY else None
        for i, (m, chunk) in enumerate(zip(ms, chunks)):
            at = f"{what} chunk {i}"
            if forced is not None and m.btype not in (forced, dt.STORED):
                bad.append(f"{at}: block type {m.btype}")
            if m.tokens is None:
                continue
            # 1. the tokens are the match rule's, whatever the block type
            if flags & LITERALS_ONLY and any(not isinstance(t, int) for t in m.tokens):
                bad.append(f"{at}: a match under LITERALS_ONLY")
            want = parse(chunk, bool(flags & LITERALS_ONLY))
            if m.tokens != want:
                k = next((j for j, (a, b) in enumerate(zip(m.tokens, want)) if a != b), min(len(m.tokens), len(want)))
                bad.append(f"{at}: token {k} is {m.tokens[k:k + 1]}, the match rule gives {want[k:k + 1]} "
                           f"({len(m.tokens)} tokens against {len(want)})")
            if any(not isinstance(t, int) and t[0] == 3 for t in m.tokens):
                bad.append(f"{at}: a match of length 3, which no candidate can give")
            # 3. the dynamic codes
            if m.btype == dt.DYNAMIC:
                _audit_codes(m, at, bad)
    # 2. the block type is the smallest by exact size
    if set(ALL) <= set(decoded):
        for i, chunk in enumerate(chunks):
            got, fixed, dyn = (decoded[f][i] for f in ALL)
            sizes = {dt.STORED: 8 * (5 + len(chunk))}
            for m in (fixed, dyn):
                if m.btype != dt.STORED:                    # (a forced type that did not fit its slot is stored)
                    sizes[m.btype] = m.coded_bits
            least = min(sizes.values())
            if got.coded_bits != least:
                bad.append(f"{name} chunk {i}: {got.coded_bits} coded bits of type {got.btype}, the sizes are {sizes}")
            elif list(sizes.values()).count(least) == 1 and sizes.get(got.btype) != least:
                bad.append(f"{name} chunk {i}: type {got.btype}, the sizes are {sizes}")
    if name == "incompressible" and 0 in decoded:
        for i, (m, chunk) in enumerate(zip(decoded[0], chunks)):
            # (the ragged tail of 17 bytes is smaller under the fixed codes, whose 8- and 9-bit literals beat 5 bytes
            # of stored header: only whole chunks must come out stored)
            if len(chunk) == C and (m.btype, m.size) != (dt.STORED, len(chunk) + 23):
                bad.append(f"{name} chunk {i}: type {m.btype}, {m.size} bytes for {len(chunk)} of text")
    return bad, decoded


def matches_of(decoded):
    """the (length, distance) pairs of every coded member of an audit's result"""
    return [t for ms in decoded.values() for m in ms if m.tokens is not None for t in m.tokens if not isinstance(t, int)]


def coverage_gaps(decoded_by_case, C):
    """4. every length symbol 258..285 and every distance symbol 0..29 (as far as the chunk size allows) comes out of the
    case built to give it: len<L> holds the match (L, 301), dist<D> a match at distance D; wide_tokens holds a token
    written into three words.  Returns the failures."""
    bad, lsyms, dsyms = [], set(), set()
    for L in LENGTH_EDGES:
        if (L, 301) in matches_of(decoded_by_case.get(f"len{L}", {})):
            lsyms.add(dt.length_symbol(L))
        else:
            bad.append(f"len{L}: no match ({L}, 301)")
    for D in DISTANCE_EDGES + FAR_DISTANCE_EDGES:
        if D + 8 > C:
            continue
        if any(t[1] == D for t in matches_of(decoded_by_case.get(f"dist{D}", {}))):
            dsyms.add(dt.distance_symbol(D))
        else:
            bad.append(f"dist{D}: no match at distance {D}")
    want_d = {dt.distance_symbol(D) for D in DISTANCE_EDGES + FAR_DISTANCE_EDGES if D + 8 <= C}
    if lsyms != set(range(258, 286)) or dsyms != want_d:
        bad.append(f"symbols not emitted: lengths {sorted(set(range(258, 286)) - lsyms)}, distances {sorted(want_d - dsyms)}")
    one = {dt.length_symbol(t[0]) for t in matches_of(decoded_by_case.get("every_length_symbol", {}))}
    if one != set(range(258, 286)):
        bad.append(f"every_length_symbol: without {sorted(set(range(258, 286)) - one)}")
    wide = [w for ms in decoded_by_case.get("wide_tokens", {}).values() for m in ms if m.tokens is not None
            for w in dt.third_word_tokens(m)]
    widest = max((w for ms in decoded_by_case.get("wide_tokens", {}).values() for m in ms if m.tokens is not None
                  for w in dt.token_offsets(m)[1]), default=0)
    print(f"wide_tokens: {len(wide)} tokens in three words, the widest token has {widest} bits")
    if not wide:
        bad.append("wide_tokens: no token is written into three words")
    return bad


if __name__ == "__main__":      # python tests/deflate_cases.py OUT [CHUNK_BYTES]
    dump_cases(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 32768)
