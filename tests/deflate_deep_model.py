"""The device gzip encoder's second effort level (PF_GZ_DEEP; csrc/pf_deflate.h: deep_length, deep_defers) as plain Python
models, and the smallest texts at which its two additions -- the previous-row candidate and the one-step lazy parse --
can go wrong.  Pure Python, no GPU: what tests/test_deflate_deep_host.py and tests/test_gpu_deflate_deep.py compare the
encoders' bytes with.  The format reader, the hashes, the match extension and match_ok are deflate_tokens', unchanged.

The rule, for a chunk of n bytes:
  A(p)  the level-1 candidate: the host model's (the last position before p with its hash4) or the kernel's (the largest
        hashed q with its hash4 and q // 8 < p // 8).
  B(p)  the same column of the row before: s = 1 + the last '\\n' before p (0: none, then no B), r = 1 + the last '\\n'
        before s - 1 (0: none), B = r + (p - s), taken only if B < s - 1.
  L(p), D(p)  both extended to MAX_MATCH, the longer, on a tie the nearer, accepted through match_ok.
  parse  at a token start q with L(q) > 0: if q + 1 < n and L(q + 1) > L(q) the literal text[q], then q + 1; else the
        match, then q + L(q)."""
import functools
import os
import random
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_tokens as dt  # noqa: E402

DEEP, BGZF = 16, 8
DEEP_FLAGS = (DEEP, DEEP | dc.FIXED_ONLY, DEEP | dc.DYNAMIC_ONLY)
NL = 10


def _cands_host(chunk):
    last, cands = {}, [None] * len(chunk)
    for p, x in enumerate(dt.hashes(chunk)):
        cands[p] = last.get(x)
        last[x] = p
    return cands


def _cands_device(chunk):
    h = dt.hashes(chunk)
    last, cands = {}, [None] * len(chunk)
    for g in range(0, len(h), 8):
        group = range(g, min(g + 8, len(h)))
        for p in group:
            cands[p] = last.get(h[p])
        for p in group:
            last[h[p]] = p
    return cands


def row_starts(chunk, drop=None):
    """(s, r) of every position; drop: the index of a '\\n' to overlook (a mutation, for `differs_from_mutants`)"""
    out, s, r = [], 0, 0
    for p, b in enumerate(chunk):
        out.append((s, r))
        if b == NL and p != drop:
            s, r = p + 1, s
    return out


def row_candidate(p, s, r):
    if s == 0:
        return None
    b = r + (p - s)
    return b if b < s - 1 else None


def _mutant_b(p, s, r, mutant):
    """candidate B under a mutation of the rule: None (the rule), "none" (no B at all), "plus1" / "minus1" (B off by one),
    "noclause" (B taken on or behind the previous row's '\\n' too)"""
    if mutant == "none":
        return None
    if mutant == "noclause":
        b = r + (p - s) if s else None
        return b if b is not None and b < p else None
    b = row_candidate(p, s, r)
    if b is None or mutant is None or isinstance(mutant, tuple):
        return b
    b += 1 if mutant == "plus1" else -1
    return b if 0 <= b < p else None


def _deep(chunk, cands, literals_only, mutant=None):
    n = len(chunk)
    rows = row_starts(chunk, mutant[1] if isinstance(mutant, tuple) else None)     # (("drop", index): a newline overlooked)
    if literals_only:
        return list(chunk)

    @functools.lru_cache(maxsize=None)
    def best(p):
        length, dist = 0, 0
        a, b = cands[p], _mutant_b(p, *rows[p], mutant)
        if a is not None:
            length, dist = dt._extend(chunk, a, p), p - a
        if b is not None and b != a:
            lb = dt._extend(chunk, b, p)
            if lb > length or (lb == length and p - b < dist):
                length, dist = lb, p - b
        return (length, dist) if dt.match_ok(length, dist) else (0, 0)

    tokens, q = [], 0
    while q < n:
        length, dist = best(q)
        if length and not (q + 1 < n and best(q + 1)[0] > length):
            tokens.append((length, dist))
            q += length
        else:
            tokens.append(chunk[q])
            q += 1
    return tokens


@functools.lru_cache(maxsize=512)
def parse_host_deep(chunk, literals_only=False):
    return _deep(chunk, _cands_host(chunk), literals_only)


@functools.lru_cache(maxsize=512)
def parse_device_deep(chunk, literals_only=False):
    return _deep(chunk, _cands_device(chunk), literals_only)


def differs_from_mutants(chunk, mutants):
    """whether the rule's tokens on `chunk`, with either table's candidate A, differ from those of every mutation named:
    a text of which this holds cannot be encoded right by a kernel or a model that makes that mistake"""
    for cands in (_cands_host(chunk), _cands_device(chunk)):
        want = _deep(chunk, cands, False)
        if any(_deep(chunk, cands, False, m) == want for m in mutants):
            return False
    return True


B_MUTANTS = ("none", "plus1", "minus1")


def deferrals(chunk, parse):
    """the positions at which the parse put a match off: a literal at q followed by a token that starts at q + 1 with a
    longer match than q had.  From the tokens and the rule's own lengths."""
    cands = _cands_host(chunk) if parse is parse_host_deep else _cands_device(chunk)
    rows, out, q = row_starts(chunk), [], 0

    def length(p):
        best = 0
        for c in (cands[p], row_candidate(p, *rows[p])):
            if c is not None:
                ln = dt._extend(chunk, c, p)
                if dt.match_ok(ln, p - c):
                    best = max(best, ln)
        return best
    for t in parse(chunk):
        if isinstance(t, int):
            if length(q):
                out.append(q)
            q += 1
        else:
            q += t[0]
    return out


# ---- the edge texts.  Rows are made of bytes 32..126 without '\n'; a "fresh" row shares no 3 bytes with anything else
def _row(seed, n):
    rng = random.Random(seed)
    return bytes(rng.randrange(33, 127) for _ in range(n))


def _distinct(seed, n):
    """n bytes in which no three bytes stand twice and no hash4 bucket is shared (drawn until so)"""
    for k in range(1000):
        t = _row(1000 * seed + k, n)
        tri = [t[i:i + 3] for i in range(n - 2)]
        if len(set(tri)) == len(tri) and len(set(dt.hashes(t))) == max(0, n - 3):
            return t
    raise AssertionError("no such bytes")


def _other(v):
    """another byte of 33..126"""
    return (v + 1) % 94 + 33


def two_rows(n):
    row = _row(n, n)
    return row + b"\n" + row + b"\n"


@functools.lru_cache(maxsize=None)
def three_byte_case(gap):
    """row 1: fresh bytes with "xyz" at column 5; `gap` bytes of a long row of other bytes would move the rows apart, so
    the distance is made by the row's own length: rows of length gap - 1 (and the '\\n'), row 2 fresh except "xyz" at
    column 5 -- its only agreement of 3 bytes with anything before it, at distance `gap`."""
    n = gap - 1
    rng = random.Random(gap)
    a = bytearray(rng.choice(b"abcdefgh") for _ in range(n))
    b = bytearray(rng.choice(b"ijklmnop") for _ in range(n))
    a[5:8] = b"XYZ"
    b[4:9] = b"qXYZr"
    return bytes(a) + b"\n" + bytes(b) + b"\n"


@functools.lru_cache(maxsize=None)
def lazy_at(q, n):
    """a text of n bytes whose parse has a deferral at position q exactly: fresh bytes, and at q a 4-byte copy of an
    earlier place whose next byte differs, while from q + 1 on 12 bytes of another earlier place are copied.  The text
    has no '\\n': both matches are candidate A's."""
    assert 64 <= q and q + 14 <= n
    for seed in range(200):
        rng = random.Random(97 * q + seed)
        t = bytearray(rng.randrange(33, 127) for _ in range(n))
        src4, src12 = 8, 32                               # (groups of eight before q's: both rules see them)
        y = bytes(t[src12:src12 + 12])
        t[src4:src4 + 4] = bytes([t[src4]]) + y[:3]       # X = x0 y0 y1 y2, then a byte that is not y3
        t[src4 + 4] = _other(y[3])
        t[src12 - 1] = _other(t[src4])                    # (nothing before Y's source that would make it X's too)
        t[q] = t[src4]
        t[q + 1:q + 13] = y
        t[q + 13] = _other(t[src12 + 12])
        text = bytes(t)
        if q in deferrals(text, parse_device_deep) and q in deferrals(text, parse_host_deep):
            return text
    raise AssertionError(f"no deferral at {q}")


@functools.lru_cache(maxsize=None)
def lazy_chain():
    """three deferrals in a row: at q, q + 1 and q + 2 a longer match starts one byte further on each time"""
    for seed in range(2000):
        rng = random.Random(seed)
        t = bytearray(rng.randrange(33, 127) for _ in range(400))
        q = 300
        # sources of growing length whose first bytes are the target's from q, q + 1, q + 2, q + 3 on
        tail = bytes(rng.randrange(33, 127) for _ in range(40))
        t[q:q + 40] = tail
        for i, (src, ln) in enumerate(((8, 4), (40, 6), (80, 9), (120, 14))):
            t[src:src + ln] = tail[i:i + ln]
            t[src + ln] = _other(tail[i + ln])
        text = bytes(t)
        for parse in (parse_device_deep, parse_host_deep):
            d = deferrals(text, parse)
            if not all(x in d for x in (q, q + 1, q + 2)):
                break
        else:
            return text
    raise AssertionError("no chain of three deferrals")


# ---- texts of rows as the files have them: "0\\t" / "1\\t" cells, every row the one before with a few cells changed.
# The hash table's candidate is then a "0\\t0\\t" a few bytes back, and only candidate B finds the long match.  Each
# builder draws until the rule's tokens differ from those of the mistakes it is there to catch (differs_from_mutants).
def cell_rows(seed, width, rows, flips=3):
    """`rows` rows of `width` bytes and their '\\n' (an odd width ends in a lone digit)"""
    rng = random.Random(seed)
    cells = [rng.choice(b"01") for _ in range((width + 1) // 2)]
    out = bytearray()
    for _ in range(rows):
        out += b"".join(bytes([c]) + b"\t" for c in cells)[:width] + b"\n"
        for _ in range(flips):
            k = rng.randrange(len(cells))
            cells[k] = cells[k] ^ 1
    return bytes(out)


def _newlines(text):
    return [i for i, b in enumerate(text) if b == NL]


def _draw(make, ok, what, tries=400):
    for seed in range(tries):
        text = make(seed)
        if ok(text):
            return text
    raise AssertionError(f"no text for {what}")


@functools.lru_cache(maxsize=None)
def rows_with_newline_at(at):
    """four rows of `at` bytes and half a fifth: the first '\\n' at index `at` -- at a step's or a wave's last and first lane for at = 255, 256,
    63, 64, .. -- and the later ones wherever 2 at + 1, .. fall.  Overlooking any one of the newlines, or a B that is
    missing or off by one, changes the tokens."""
    def ok(text):
        return differs_from_mutants(text, B_MUTANTS + tuple(("drop", i) for i in _newlines(text)))
    return _draw(lambda seed: cell_rows(1000 * at + seed, at, 5)[:-(at // 2) - 1], ok, f"newline at {at}")


@functools.lru_cache(maxsize=None)
def long_cell_rows():
    """rows of 330 bytes behind a short one: a row's start, and the start of the row before it, lie in earlier steps"""
    def ok(text):
        return differs_from_mutants(text, B_MUTANTS + tuple(("drop", i) for i in _newlines(text)))
    return _draw(lambda seed: b"0\t\n" + cell_rows(seed, 330, 5)[:-100], ok, "long rows")


@functools.lru_cache(maxsize=None)
def equal_cell_rows():
    """two equal rows of 300 bytes and 200 bytes of a third: the match at distance 301 is longer than MAX_MATCH, and B
    alone finds it"""
    def make(seed):
        row = cell_rows(seed, 300, 1)
        return row + row + row[:200]

    def ok(text):
        return differs_from_mutants(text, B_MUTANTS) and all((258, 301) in parse(text) for parse in (parse_host_deep, parse_device_deep))
    return _draw(make, ok, "equal rows")


@functools.lru_cache(maxsize=None)
def unequal_cell_rows():
    """a row of 21 bytes, then rows of 66 made of one 22-byte unit three times: from column 21 on the second row has no B
    (it would fall on or behind the first row's '\\n') -- and a B taken there all the same, 22 bytes back, would match to
    the row's end.  The third and fourth rows have their B again."""
    def make(seed):
        unit = cell_rows(seed, 22, 1)[:22]
        body = cell_rows(seed + 7, 66, 2)
        return cell_rows(seed + 3, 21, 1) + unit * 3 + b"\n" + body

    def ok(text):
        return differs_from_mutants(text, B_MUTANTS + ("noclause",))
    return _draw(make, ok, "unequal rows")


@functools.lru_cache(maxsize=None)
def newline_first_only():
    """'\\n' at byte 0 only: s = 1 everywhere and no position has a B -- one taken all the same would be the byte before"""
    rng = random.Random(2)
    return _draw(lambda seed: b"\n" + bytes(rng.choice(b"01\t") for _ in range(500)),
                 lambda text: differs_from_mutants(text, ("noclause",)), "newline first")


@functools.lru_cache(maxsize=None)
def lazy_through_b_at(q):
    """a deferral at position q, a step's last, whose longer match at q + 1 is candidate B's: the walking lane needs the row
    starts of the next step's first position.  In these rows a changed cell's digit has a short match from the table and
    the tab behind it the rest of the row from B."""
    def ok(text):
        rows = row_starts(text)
        for parse in (parse_host_deep, parse_device_deep):
            if q not in deferrals(text, parse):
                return False
            at, after = 0, None
            for t in parse(text):
                if at == q + 1:
                    after = t
                at += 1 if isinstance(t, int) else t[0]
            b = row_candidate(q + 1, *rows[q + 1])
            if b is None or isinstance(after, int) or after is None or after[1] != q + 1 - b:
                return False
        return differs_from_mutants(text, B_MUTANTS + tuple(("drop", i) for i in _newlines(text) if i <= q))
    return _draw(lambda seed: cell_rows(seed, 90 + seed % 50, 8, flips=4)[:-30], ok, f"a deferral through B at {q}", 4000)


def deep_cases(C):
    """(name, text): each a chunk or two at most"""
    real = dc.real_shapes(C)
    yield "no_newline", _row(1, 700)
    yield "newline_first", newline_first_only()
    yield "newline_last", cell_rows(3, 700, 1)
    yield "only_newlines", b"\n" * (C + 5)
    yield "only_newlines_short", b"\n" * 700
    yield "long_rows", long_cell_rows()
    for at in (63, 64, 191, 192, 255, 256, 257):
        yield f"newline_at_{at}", rows_with_newline_at(at)
    yield "equal_rows_300", equal_cell_rows()
    yield "unequal_rows", unequal_cell_rows()
    yield "three_bytes_near", three_byte_case(4096)
    yield "three_bytes_far", three_byte_case(4097)
    yield "lazy_at_255", lazy_at(255, 700)
    yield "lazy_at_511", lazy_at(511, 700)
    yield "lazy_through_b_at_255", lazy_through_b_at(255)
    yield "lazy_through_b_at_511", lazy_through_b_at(511)
    yield "lazy_at_n_minus_2", _lazy_end()
    yield "lazy_chain", lazy_chain()
    equal = cell_rows(9, 127, 1) * 2
    yield "equal_rows_over_a_chunk", (equal * (C // len(equal) + 2))[:C + 1]
    for name, text in real.items():
        yield f"shape_{name}", text


@functools.lru_cache(maxsize=None)
def _lazy_end():
    """L(q + 1) > L(q) with q = n - 2 cannot be: L(n - 1) is at most 1, and a match is 3 bytes or more.  The nearest the
    rule allows is the deferral whose longer match ends the text, q + 1 + L(q + 1) = n, with the shortest lengths there
    are: L(q) = 3 by candidate B, L(q + 1) = 4 by candidate A, q = n - 5 -- the walk's look at q + 1 and the match's
    extension both stop at the chunk's last byte."""
    for seed in range(200):
        rng = random.Random(seed)
        row = bytearray(rng.randrange(33, 127) for _ in range(40))
        nxt = bytearray(rng.randrange(33, 127) for _ in range(40))
        nxt[35:38] = row[35:38]
        nxt[38] = _other(row[38])
        row[10:14] = nxt[36:40]
        text = bytes(row) + b"\n" + bytes(nxt)
        q = len(text) - 5
        if q in deferrals(text, parse_device_deep) and q in deferrals(text, parse_host_deep):
            return text
    raise AssertionError("no deferral at the text's end")


def segment_case(C):
    """a text of two segments whose first has an odd length and ends inside a row: the second segment's first chunk starts
    inside a row.  (text, segment ends)"""
    text = dc.real_shapes(C)["hashes_to_patterns"][:C + 999]
    return text, [4321, len(text)]


def audit_deep(name, data, encode, parse, C, flagset=dc.ALL):
    """deflate_cases.audit at level 2: `encode(data, flags)` is given the case's flags and adds DEEP itself, so that the
    audit sees its own three flag sets and checks the block choice too.  One of audit's findings does not hold at this
    level and is replaced: a match of length 3 is no failure here (candidate B can give one), but one further than
    4 096 bytes back is."""
    bad, decoded = dc.audit(name, data, flagset, encode, parse, C)
    bad = [b for b in bad if not b.endswith("a match of length 3, which no candidate can give")]
    for flags, ms in decoded.items():
        for i, m in enumerate(ms):
            if m.tokens is not None and any(not isinstance(t, int) and t[0] == 3 and t[1] > 4096 for t in m.tokens):
                bad.append(f"{name}-f{flags} chunk {i}: a match of length 3 more than 4 096 bytes back")
    return bad, decoded


def member_sizes(raw, head=10):
    """the sizes of the members of a stream, by zlib (wbits 31 takes a BGZF head too)"""
    sizes, at = [], 0
    while at < len(raw):
        z = zlib.decompressobj(31)
        piece = raw[at:at + (1 << 17)]
        z.decompress(piece)
        assert z.eof
        sizes.append(len(piece) - len(z.unused_data))
        at += sizes[-1]
    return sizes


def zlib_total(data, C, level, frame=0):
    """the bytes of the same cuts as gzip members made by zlib at `level`: raw deflate plus the 18 bytes of a member's
    head and tail, plus `frame` per member"""
    total = 0
    for chunk in dc.chunks_of(data, C):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(z.compress(chunk) + z.flush()) + 18 + frame
    return total


# the zlib level the level-2 total on hashes_to_patterns is held against: the highest of 1, 4, 6, 9 that the host model
# beats by at least 2 %, measured before the kernel was written (profiles/gzip_deep/README.md)
ZLIB_LEVEL = 4
