"""Hand-made deflate streams for the device gunzip (tests/test_inflate_edges_host.py on the CPU, tests/test_gpu_inflate_edges.py
on the GPU): the corners of RFC 1951 that neither zlib nor this project's encoder writes -- a lone distance code, a block
without one, codes of 15 bits, every length and distance symbol at its first and last value, length 258 as symbol 284,
overlapped copies around the wave's width, run codes across the literal/length and distance lengths, tables that follow
one another inside a member, stored blocks at every bit offset -- and the streams that must be refused, each with the
status it must report.  A writer goes from tokens to bits; zlib is the reference: every accepted body gives its text under
zlib.decompressobj(-15) and every refused body is refused by zlib (or, where only the container refuses it, taken) before
it is used.  A seeded generator adds members of random tokens under random complete codes.  Pure Python, no GPU.

Frames: "plain" (the 10-byte head, one member), "bgzf" (a BGZF member and the end marker) and "bgzf64" (the same blocks
behind a non-final stored lead of more than C bytes, so that the member's text exceeds C and gz_inflate64_kernel takes it).
C is pf_gzip_device_chunk_bytes()."""
import bisect
import collections
import os
import random
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgzf_cases as bc  # noqa: E402
import deflate_tokens as dt  # noqa: E402
import inflate_cases as ic  # noqa: E402

FIXED_LL_CODES = ic.canonical(dt.FIXED_LL)               # all 288 symbols, 286 and 287 among them
FIXED_D_CODES = {s: (s, 5) for s in range(32)}
RUN_EXTRA = {16: 2, 17: 3, 18: 7}
RUN_BASE = {16: 3, 17: 3, 18: 11}
SEED, N_RANDOM = 20260, 200                              # of random_members(): the set the tests use


# ---- blocks.  A token is an int literal, (length, distance), (length, distance, length symbol) -- to write 258 as symbol
# 284 with extra 31 --, or, for streams that must be refused: ("ll", symbol) / ("d", symbol), that code alone,
# ("bits", value, n), n raw bits, and ("far", length, distance), a match whose distance need not lie in the text.
def stored(data, final):
    return {"type": dt.STORED, "final": final, "data": bytes(data)}


def fixed(tokens, final, eob=True):
    return {"type": dt.FIXED, "final": final, "tokens": list(tokens), "eob": eob}


def dynamic(tokens, ll_lens, d_lens, final, header_symbols=None, hlit=None, hdist=None, cl_lens=None, eob=True, check_header=True):
    """header_symbols: [(code-length symbol, extra value)] in place of the lengths one by one; hlit / hdist: the counts
    the header declares, where they are not len(ll_lens) / len(d_lens); cl_lens: the 19 lengths of the code-length code"""
    return {"type": dt.DYNAMIC, "final": final, "tokens": list(tokens), "ll": list(ll_lens), "d": list(d_lens),
            "header": header_symbols, "hlit": hlit, "hdist": hdist, "cl": cl_lens, "eob": eob, "check": check_header}


def one_by_one(lens):
    return [(n, 0) for n in lens]


def expand_header(symbols):
    """the lengths a list of code-length symbols stands for"""
    lens = []
    for sym, extra in symbols:
        if sym < 16:
            lens.append(sym)
        else:
            assert 0 <= extra < 1 << RUN_EXTRA[sym] and (sym != 16 or lens)
            lens += [lens[-1] if sym == 16 else 0] * (RUN_BASE[sym] + extra)
    return lens


def length_code(length, forced=None):
    """(symbol, extra value, extra bits)"""
    ls = forced if forced is not None else dt.length_symbol(length)
    eb = dt.LENGTH_EXTRA[ls - 257]
    ev = length - dt.LENGTH_BASE[ls - 257]
    assert 0 <= ev < 1 << eb or (eb == 0 and ev == 0), (length, ls)
    return ls, ev, eb


def distance_code(dist):
    ds = dt.distance_symbol(dist)
    ev = dist - dt.DIST_BASE[ds]
    assert 0 <= ev < max(1, 1 << dt.DIST_EXTRA[ds]), dist
    return ds, ev, dt.DIST_EXTRA[ds]


def distance_range(sym):
    return dt.DIST_BASE[sym], dt.DIST_BASE[sym] + (1 << dt.DIST_EXTRA[sym]) - 1


Written = collections.namedtuple("Written", "body text marks nbits header_ends widths")


def write(blocks):
    """the raw deflate bytes of `blocks` and their text by plain byte-serial expansion.  marks: (text offset, block, token)
    of every token that gives text, in order; nbits: the stream's bits before its last byte is filled up; header_ends:
    the bit position behind each block's BFINAL and BTYPE; widths: the code lengths of the literal/length and distance
    symbols the tokens used, as (alphabet, symbol, bits)"""
    parts, b, done = [], ic.Bits(), 0
    text, marks, header_ends, widths = bytearray(), [], [], set()
    for bi, blk in enumerate(blocks):
        b.put(1 if blk["final"] else 0, 1).put(blk["type"], 2)
        header_ends.append(done + b.n)
        if blk["type"] == dt.STORED:
            data = blk["data"]
            assert len(data) <= 65535
            b.align().put(len(data), 16).put(len(data) ^ 0xFFFF, 16)
            parts += [b.bytes(), data]
            done += b.n + 8 * len(data)
            b = ic.Bits()
            if data:
                marks.append((len(text), bi, ("stored", len(data))))
            text += data
            continue
        if blk["type"] == dt.FIXED:
            ll, d = FIXED_LL_CODES, FIXED_D_CODES
        else:
            ll, d = ic.canonical(blk["ll"]), ic.canonical(blk["d"])
            cl_lens = blk["cl"] or ic.CL_LENGTHS
            cl = ic.canonical(cl_lens)
            header = blk["header"] if blk["header"] is not None else one_by_one(blk["ll"] + blk["d"])
            if blk["check"]:
                assert expand_header(header) == blk["ll"] + blk["d"], "the header's symbols are not the block's lengths"
            b.put((blk["hlit"] or len(blk["ll"])) - 257, 5).put((blk["hdist"] or len(blk["d"])) - 1, 5).put(19 - 4, 4)
            for s in dt.CL_ORDER:
                b.put(cl_lens[s], 3)
            for sym, extra in header:
                b.code(*cl[sym])
                if sym >= 16:
                    b.put(extra, RUN_EXTRA[sym])
        for tok in blk["tokens"]:
            if isinstance(tok, int):
                b.code(*ll[tok])
                widths.add(("ll", tok, ll[tok][1]))
                marks.append((len(text), bi, tok))
                text.append(tok)
            elif tok[0] == "ll":
                b.code(*ll[tok[1]])
            elif tok[0] == "d":
                b.code(*d[tok[1]])
            elif tok[0] == "bits":
                b.put(tok[1], tok[2])
            elif tok[0] == "far":                                       # a match that is written and not expanded
                (ls, lev, leb), (ds, dev, deb) = length_code(tok[1]), distance_code(tok[2])
                b.code(*ll[ls]).put(lev, leb).code(*d[ds]).put(dev, deb)
            else:
                length, dist = tok[0], tok[1]
                ls, lev, leb = length_code(length, tok[2] if len(tok) > 2 else None)
                ds, dev, deb = distance_code(dist)
                b.code(*ll[ls]).put(lev, leb).code(*d[ds]).put(dev, deb)
                widths.update((("ll", ls, ll[ls][1]), ("d", ds, d[ds][1])))
                assert dist <= len(text), (tok, len(text))
                marks.append((len(text), bi, tok))
                for _ in range(length):
                    text.append(text[-dist])
        if blk["eob"]:
            b.code(*ll[256])
            widths.add(("ll", 256, ll[256][1]))
    parts.append(b.bytes())
    return Written(b"".join(parts), bytes(text), marks, done + b.n, header_ends, widths)


def token_at(marks, offset):
    """the (text offset, block, token) that wrote text[offset]"""
    return marks[bisect.bisect_right([m[0] for m in marks], offset) - 1]


def first_difference(got, text, marks):
    """where `got` leaves `text`, and the token that wrote that byte, for a failure's message"""
    if got is None:
        return "not taken"
    n = next((i for i in range(min(len(got), len(text))) if got[i] != text[i]), min(len(got), len(text)))
    if n == len(got) == len(text):
        return None
    if n >= len(text):
        return f"{len(got)} bytes for {len(text)}"
    at, block, tok = token_at(marks, n)
    what = f"(len {tok[0]}, dist {tok[1]})" if isinstance(tok, tuple) and tok[0] != "stored" else repr(tok)
    return f"offset {n} differs: byte {n - at} of token {what} at {at} in block {block}"


# ---- the reference
def zlib_inflate(body):
    """(text, None) where zlib takes exactly `body`, else (None, why)"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(body)
    except zlib.error as e:
        return None, str(e)
    if not d.eof:
        return None, "incomplete"
    return (text, None) if not d.unused_data else (None, "unused data")


# ---- codes
def flat(size, symbols):
    """`size` lengths: a complete code over `symbols`, as even as it gets (one symbol: one bit)"""
    symbols, lens = list(symbols), [0] * size
    n = len(symbols)
    k = max(1, n.bit_length() - 1)
    short = (1 << (k + 1)) - n if n > 1 else 1
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    assert n == 1 or dt.kraft(lens) == 1 << dt.MAX_BITS
    return lens


def ladder(size, symbols):
    """a complete code of lengths 1, 2, ..., n - 1, n - 1 over the n symbols, in their order"""
    symbols, lens = list(symbols), [0] * size
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    assert dt.kraft(lens) == 1 << dt.MAX_BITS
    return lens


FULL_LL = flat(286, range(286))           # all 286 lengths present: 226 of 8 bits, 60 of 9
FULL_D = flat(30, range(30))              # all 30: 2 of 4 bits, 28 of 5


# ---- the accepted cases.  A maker takes the bytes of text in front of its blocks (`before`: 0, or the large frame's
# lead) and the bytes of text it may give (`room`), and returns its blocks; what a case is for is asserted where it is made.
def _one_dist_block(final, first=None):
    ll = flat(286, [97, 120, 256, 258, 285])                           # 'a', 'x', end of block, lengths 4 and 258
    toks = ([first] if first else []) + [120, (4, 1), 120, 97, (258, 1), (4, 1)]
    return dynamic(toks, ll, [1], final)


def one_dist_code_1bit(before, room):
    blk = _one_dist_block(True, first=97)
    assert blk["d"] == [1] and sum(isinstance(t, tuple) for t in blk["tokens"]) == 3
    return [blk]


def no_dist_code_literals(before, room):
    toks = list(b"no distance code at all\n")
    blk = dynamic(toks, flat(257, sorted(set(toks)) + [256]), [0], True)
    assert blk["d"] == [0] and all(isinstance(t, int) for t in toks)
    return [blk]


def only_eob_code_then_fixed(before, room):
    ll = [0] * 257
    ll[256] = 1
    return [dynamic([], ll, [0], False), fixed(list(b"abc") + [(6, 3), 100], True)]


def codes_of_15_bits_ll(before, room):
    ll = ladder(258, list(b"abcdefghijkl") + [257, 256, 121, 122])       # 'y' and 'z' take the two codes of 15 bits
    assert sorted(n for n in ll if n) == list(range(1, 15)) + [15, 15] and ll[121] == ll[122] == 15
    toks = list(b"abcabclkz") + [(3, 2), 121, 122, 121, (3, 1), 122]
    return [dynamic(toks, ll, [1, 1], True)]


def _lead_text(n, seed):
    return bc.tsv_text(n, seed=seed)


def codes_of_15_bits_dist(before, room):
    lead = _lead_text(min(room - 64, 24600), 21)
    top = dt.distance_symbol(len(lead))
    assert top >= 15
    syms = list(range(top - 15, top + 1))                                # the two highest usable symbols take 15 bits
    d = ladder(top + 1, syms)
    assert sorted(n for n in d if n) == list(range(1, 15)) + [15, 15] and d[top] == d[top - 1] == 15
    if len(lead) >= 24577:
        assert (top - 1, top) == (28, 29)
    toks = [65]
    for s in (top, top - 1, syms[0], top, syms[3], top - 1):
        first, last = distance_range(s)
        toks += [(5, first), 66, (4, min(last, len(lead)))]
    return [stored(lead, False), dynamic(toks, flat(286, [65, 66, 256, 258, 259]), d, True)]


def _eob_15(other, unused):
    """the end-of-block code is one of the two of 15 bits (`other` is the second) and `unused` bits of the payload's
    last byte stay free: one-bit literals in front move it there"""
    def maker(before, room):
        ll = ladder(max(257, other) + 1, list(b"abcdefghijklmn") + sorted([256, other]))
        assert ll[256] == 15 and ll[97] == 1
        for pad in range(8):
            blocks = [dynamic([97] * pad + list(b"abcdefghijklmnaa"), ll, [1, 1], True)]
            if (8 - write(blocks).nbits % 8) % 8 == unused:
                return blocks
        raise AssertionError("no padding puts the end-of-block code there")
    return maker


def len_258_by_284(before, room):
    toks = list(b"ab") + [(258, 2, 284), 99, (258, 1, 284), (258, 259), (257, 1)]
    assert length_code(258, 284) == (284, 31, 5)
    return [fixed(toks, True)]


def _extremes_tokens(reach):
    """one match per length symbol at its first and last length, then one per distance symbol at its first and last
    distance no larger than `reach`, the text in front of the first of them.  (tokens, the pairs emitted)"""
    toks, pairs = [], set()
    for i, sym in enumerate(range(257, 286)):
        for which, length in zip(("first", "last"), dt.length_range(sym)):
            dist = (1, length - 1, length, length + 1, 64, 3)[(2 * i + (which == "last")) % 6]
            toks += [(length, max(1, dist), sym), 48 + i % 10]
            pairs.add(("len", sym, which))
    for sym in range(30):
        for which, dist in zip(("first", "last"), distance_range(sym)):
            if dist <= reach:
                toks += [(4, dist), 97 + sym % 26]
                pairs.add(("dist", sym, which))
    return toks, pairs


def _extremes(block_of):
    def maker(before, room):
        probe, _ = _extremes_tokens(0)
        need = sum(t[0] if isinstance(t, tuple) else 1 for t in probe) + 30 * 2 * 5
        lead = b"" if before >= 32768 else _lead_text(room - need, 22)
        reach = before + len(lead) + need - 30 * 2 * 5
        toks, pairs = _extremes_tokens(reach)
        want = {("len", s, w) for s in range(257, 286) for w in ("first", "last")}
        want |= {("dist", s, w) for s in range(30) for w, d in zip(("first", "last"), distance_range(s)) if d <= reach}
        assert pairs == want
        if reach >= 24577:
            assert ("dist", 29, "first") in pairs
        if before >= 32768:
            assert len(pairs) == 2 * 29 + 2 * 30
        return ([stored(lead, False)] if lead else []) + [block_of(toks)]
    return maker


def overlap_grid_distances():
    return list(range(1, 70)) + [127, 128, 129]


def overlap_grid_lengths(dist):
    return sorted({min(258, max(3, n)) for n in (3, dist - 1, dist, dist + 1, 63, 64, 65, 128, 129, 258)})


def overlap_grid_tokens(dists):
    """a 128-byte lead of distinct bytes, then every (dist, len) of the grid with one literal between two matches that
    differs from its neighbours; (tokens, the pairs, bytes of text)"""
    toks, pairs, n = list(range(128)), [], 128
    for dist in dists:
        for length in overlap_grid_lengths(dist):
            toks += [128 + len(pairs) % 127, (length, dist)]
            pairs.append((dist, length))
            n += 1 + length
    return toks, pairs, n


def overlap_grid_groups(limit):
    """the grid's distances in as few runs as give at most `limit` bytes of text each"""
    groups, cur = [], []
    for dist in overlap_grid_distances():
        if cur and overlap_grid_tokens(cur + [dist])[2] > limit:
            groups.append(cur)
            cur = []
        cur.append(dist)
    return groups + [cur]


def _grid(dists):
    def maker(before, room):
        toks, pairs, n = overlap_grid_tokens(dists)
        assert n <= room and set(pairs) == {(d, ln) for d in dists for ln in overlap_grid_lengths(d)}
        return [fixed(toks, True)]
    return maker


GRID_LARGE = [1, 2, 3, 31, 32, 33] + list(range(60, 70)) + [127, 128, 129]        # the large frame's one grid member


def repeat_16_across_ll_dist(before, room):
    ll = [0] * 260
    ll[97], ll[256], ll[257], ll[258], ll[259] = 1, 2, 3, 4, 4
    d = [4, 4, 3, 2, 1]
    header = one_by_one(ll[:259]) + [(16, 0)] + one_by_one(d[2:])      # one code 16: ll[259], d[0], d[1]
    assert expand_header(header) == ll + d and header[259] == (16, 0)
    toks = [97] * 9 + [(5, 1), (4, 2), 97, (3, 3), (5, 4), (3, 5), (4, 6), 97]    # every symbol the two codes have
    return [dynamic(toks, ll, d, True, header_symbols=header)]


def repeat_16_after_17(before, room):
    """a code 16 behind a code 17 repeats the zero, not the length in front of the 17"""
    ll = flat(257, [0, 97, 256])
    header = [(ll[0], 0), (17, 0), (16, 3), (18, 97 - 10 - 11)] + one_by_one(ll[97:98]) + [(18, 138 - 11), (18, 256 - 236 - 11), (ll[256], 0), (1, 0), (1, 0)]
    assert expand_header(header) == ll + [1, 1] and header[:3] == [(1, 0), (17, 0), (16, 3)]
    return [dynamic([0, 97, 97, 0], ll, [1, 1], True, header_symbols=header)]


def repeat_18_of_138(before, room):
    ll = flat(258, [97, 236, 256, 257])
    header = [(18, 97 - 11), (ll[97], 0), (18, 127), (ll[236], 0), (18, 19 - 11), (ll[256], 0), (ll[257], 0), (1, 0), (1, 0)]
    assert expand_header(header) == ll + [1, 1] and (18, 127) in header
    return [dynamic([97, 236, (3, 2), 97], ll, [1, 1], True, header_symbols=header)]


def hlit_257_hdist_1_after_full(before, room):
    first = dynamic(list(b"abcabcab") + [(4, 3), 99], FULL_LL, FULL_D, False)
    ll = [0] * 257
    ll[97], ll[98], ll[99], ll[256] = 1, 2, 3, 3                          # symbols the first block had at 8 bits
    second = dynamic(list(b"cabac"), ll, [0], False)                      # (no length code: this block cannot hold a match)
    assert all(FULL_LL[s] != ll[s] for s in (97, 98, 99, 256)) and len(FULL_LL + FULL_D) == 316
    third = fixed([(12, 5 + 9), 100, (5, 1)], False)                     # through the second block's text into the first's
    fourth = _one_dist_block(True)
    fourth["tokens"] = [(4, 1)] + fourth["tokens"]                        # into the third block's last byte
    return [first, second, third, fourth]


def _stored_at_bit_offset(k):
    def maker(before, room):
        # 3 + 8a + 9b + 7 bits of a fixed block, 3 of the next block's header: (5 + b) % 8 == k
        lits = list(b"xyz") + [200] * ((k - 5) % 8)
        blocks = [fixed(lits, False), stored(b"0123456789", False), fixed([(7, 9), 33, (3, 1)], True)]
        assert write(blocks).header_ends[1] % 8 == k
        return blocks
    return maker


def stored_len_0_final(before, room):
    return [fixed(list(b"abc") + [(5, 3)], False), stored(b"", True)]


def _makers(C, large):
    out = [("one_dist_code_1bit", one_dist_code_1bit), ("no_dist_code_literals", no_dist_code_literals),
           ("only_eob_code_then_fixed", only_eob_code_then_fixed), ("codes_of_15_bits_ll", codes_of_15_bits_ll),
           ("codes_of_15_bits_dist", codes_of_15_bits_dist), ("eob_of_15_bits_ends_the_payload", _eob_15(122, 0)),
           ("eob_of_15_bits_then_7_unused_bits", _eob_15(257, 7)), ("len_258_by_284", len_258_by_284),
           ("every_symbol_extremes", _extremes(lambda toks: fixed(toks, True))),
           ("hlit_286_hdist_30", _extremes(lambda toks: dynamic(toks, FULL_LL, FULL_D, True)))]
    if large:
        out.append(("overlap_grid_beyond_32768", _grid(GRID_LARGE)))
    else:
        out += [(f"overlap_grid_{g[0]}_to_{g[-1]}", _grid(g)) for g in overlap_grid_groups(min(C, 24576))]
    out += [("repeat_16_across_ll_dist", repeat_16_across_ll_dist), ("repeat_16_after_17", repeat_16_after_17),
            ("repeat_18_of_138", repeat_18_of_138), ("hlit_257_hdist_1_after_full", hlit_257_hdist_1_after_full)]
    out += [(f"stored_at_bit_offset_{k}", _stored_at_bit_offset(k)) for k in range(8)]
    out.append(("stored_len_0_final", stored_len_0_final))
    return out


Case = collections.namedtuple("Case", "name frame data text marks widths")
FRAMES = ("plain", "bgzf", "bgzf64")


def large_lead(C):
    return _lead_text(max(C + 1, 32768 + 1), 11)


def framed(name, frame, blocks, C):
    """the blocks in a frame, after zlib has agreed with the writer's text"""
    w = write(blocks)
    got, why = zlib_inflate(w.body)
    assert got == w.text, f"{name} ({frame}): zlib: {why or 'another text'}"
    if frame == "plain":
        assert len(w.text) <= C and 18 + len(w.body) <= ic.slot_bytes(C), name
        data = ic.wrap(w.body, w.text)
    else:
        assert (len(w.text) <= C) == (frame == "bgzf"), name
        data = bc.frame(w.body, w.text) + bc.EOF
    return Case(name, frame, data, w.text, w.marks, w.widths)


def accepted(C):
    """[Case]: every case in the plain, the BGZF and the large BGZF frame"""
    out, lead = [], large_lead(C)
    for frame in FRAMES:
        before, room = (len(lead), bc.MAX - len(lead)) if frame == "bgzf64" else (0, C)
        for name, maker in _makers(C, frame == "bgzf64"):
            blocks = maker(before, room)
            out.append(framed(name, frame, ([stored(lead, False)] if before else []) + blocks, C))
    # what the named cases are for, read back from what was written
    by = {(c.name, c.frame): c for c in out}
    for frame in FRAMES:
        assert ("ll", 121, 15) in by["codes_of_15_bits_ll", frame].widths and ("ll", 122, 15) in by["codes_of_15_bits_ll", frame].widths
        assert sum(1 for a, s, n in by["codes_of_15_bits_dist", frame].widths if a == "d" and n == 15) == 2
        assert ("ll", 256, 15) in by["eob_of_15_bits_ends_the_payload", frame].widths
        assert any(len(t) == 3 and t[:1] == (258,) and t[2] == 284 for _, _, t in by["len_258_by_284", frame].marks if isinstance(t, tuple))
    seen = {(t[1], t[0]) for c in out if c.name.startswith("overlap_grid") and c.frame == "plain" for _, _, t in c.marks if isinstance(t, tuple)}
    assert seen == {(d, ln) for d in overlap_grid_distances() for ln in overlap_grid_lengths(d)}
    grid64 = by["overlap_grid_beyond_32768", "bgzf64"]
    assert min(at for at, _, t in grid64.marks if isinstance(t, tuple) and t[0] != "stored") > 32768
    return out


# ---- the refused cases
Refused = collections.namedtuple("Refused", "name frame data member reason")


def _ll3():
    ll = [0] * 258
    ll[97], ll[256], ll[257] = 1, 2, 2
    return ll


def _refused_bodies(C):
    """[(name, body, the text its tail is made of, the status, what zlib says of the bare body: "error", "incomplete" or
    "takes")]"""
    out = []

    def add(name, blocks, reason, zl="error", tail_text=b"?" * 64):        # (a tail that leaves room: the stream is refused first)
        out.append((name, write(blocks).body, tail_text, reason, zl))

    pad = [("bits", 0, 7), ("bits", 0, 24)]                               # (at least two more payload bytes)
    # a lone distance code of one bit is the bit 0: the bit 1 is no code.  Behind 15 or more bits of payload that is
    # "bad code"; within the payload's last 15 bits the decoder cannot tell it from a code cut short: "truncated"
    lone = [97, ("ll", 257), ("bits", 1, 1)]
    add("one_dist_code_other_bit", [dynamic(lone + pad, _ll3(), [1], True, eob=False)], "bad code")
    add("one_dist_code_other_bit_at_the_end", [dynamic(lone, _ll3(), [1], True, eob=False)], "truncated")
    none = [97, ("ll", 257), ("bits", 0, 1)]
    add("match_without_dist_code", [dynamic(none + pad, _ll3(), [0], True, eob=False)], "bad code")
    add("match_without_dist_code_at_the_end", [dynamic(none, _ll3(), [0], True, eob=False)], "truncated")
    # (with the tail of the text they would give: only the code's refusal keeps these two from being taken)
    add("lone_dist_code_2bits", [dynamic([97], _ll3(), [2], True)], "bad code", tail_text=b"a")
    ll = [0] * 257
    ll[256] = 2
    add("lone_eob_code_2bits", [dynamic([], ll, [0], True)], "bad code", tail_text=b"")
    ll = [0] * 257
    ll[97] = ll[98] = 1
    add("no_eob_code", [dynamic([97], ll, [1, 1], True, eob=False)], "bad code")
    cl = [0] * 19
    cl[0] = cl[1] = 2
    add("cl_code_incomplete", [dynamic([], [0] * 257, [0], True, cl_lens=cl, header_symbols=[(0, 0)] * 258, eob=False)], "bad code")
    cl = [0] * 19
    cl[0] = 1
    add("cl_code_one_symbol", [dynamic([], [0] * 257, [0], True, cl_lens=cl, header_symbols=[(0, 0)] * 258, eob=False)], "bad code")
    for sym in (286, 287):
        add(f"fixed_length_symbol_{sym}", [fixed([97, ("ll", sym), ("d", 0)] + pad, True)], "bad symbol")
    for sym in (30, 31):
        add(f"fixed_distance_symbol_{sym}", [fixed([97, 98, 99, ("ll", 257), ("d", sym)] + pad, True)], "bad symbol")
    ok = dynamic([97, (3, 1)], _ll3(), [1, 1], True)
    assert zlib_inflate(write([ok]).body) == (b"aaaa", None)                # the block the four below spoil
    add("hlit_287", [dict(ok, hlit=287)], "bad code lengths")
    add("hlit_288", [dict(ok, hlit=288)], "bad code lengths")
    add("hdist_31", [dict(ok, hdist=31)], "bad code lengths")
    add("hdist_32", [dict(ok, hdist=32)], "bad code lengths")
    lens = _ll3() + [1, 1]
    add("repeat_past_end", [dict(ok, header=one_by_one(lens[:-2]) + [(16, 3)], check=False)], "bad code lengths")
    ll = [0] * 257
    ll[256] = 1
    header = [(18, 127), (18, 256 - 138 - 11), (1, 0), (18, 0)]           # the last run: 11 zeros where 10 lengths are left
    add("repeat_18_past_end_by_one", [dynamic([], ll, [0] * 10, True, header_symbols=header, check_header=False)], "bad code lengths")
    assert len(expand_header(header)) == 257 + 10 + 1
    good = write([fixed(list(b"abc") + [(5, 3)], True)])
    out.append(("byte_before_tail", good.body + b"\0", good.text, "ends before its tail", "takes"))
    for o in (3, 300):
        lead = list(_lead_text(o, 23))
        add(f"dist_one_too_far_behind_{o}", [fixed(lead + [("far", 3, o + 1)], True)], "distance before the start", tail_text=bytes(lead) + b"???")
    add("len_one_past_isize", [fixed(list(b"abc") + [(5, 3)], True)], "more text than ISIZE", zl="takes", tail_text=good.text[:-1])
    return out


def refused(C):
    """[Refused]: every case in the plain and the BGZF frame, alone (member 0) and between two good members (member 1)"""
    good = write([fixed(list(b"a good member\n") + [(14, 14)], True)])
    assert zlib_inflate(good.body)[0] == good.text
    out = []
    for name, body, tail_text, reason, zl in _refused_bodies(C):
        bare = body[:-1] if name == "byte_before_tail" else body
        got, why = zlib_inflate(bare)
        if zl == "takes":
            assert got is not None, name
        else:
            assert got is None and (why == "incomplete") == (zl == "incomplete"), (name, why)
        plain, bgzf = ic.wrap(body, tail_text), bc.frame(body, tail_text)
        gp, gb = ic.wrap(good.body, good.text), bc.frame(good.body, good.text)
        out += [Refused(name, "plain", plain, 0, reason), Refused(name, "bgzf", bgzf + bc.EOF, 0, reason),
                Refused(name + "_between_good_ones", "plain", gp + plain + gp, 1, reason),
                Refused(name + "_between_good_ones", "bgzf", gb + bgzf + gb + bc.EOF, 1, reason)]
    return out


# ---- the seeded generator
def random_complete_lengths(rng, size, symbols):
    """a random complete code over `symbols`: a random full binary tree's leaf depths, capped at 15 -- a leaf is split in
    two until there are as many leaves as symbols, half the time the deepest one that may still be split"""
    symbols, lens = list(symbols), [0] * size
    if len(symbols) == 1:
        lens[symbols[0]] = 1
        return lens
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        can = [i for i, n in enumerate(leaves) if n < dt.MAX_BITS]
        i = max(can, key=lambda j: leaves[j]) if rng.random() < 0.5 else rng.choice(can)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    for s, n in zip(symbols, leaves):
        lens[s] = n
    assert dt.kraft(lens) == 1 << dt.MAX_BITS
    return lens


def random_runs(rng, lens):
    """the lengths as code-length symbols, a run code wherever a run allows one and the draw says so"""
    out, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and rng.random() < 0.8:
            if run >= 11 and rng.random() < 0.7:
                r = rng.randint(11, min(run, 138))
                out.append((18, r - 11))
            else:
                r = rng.randint(3, min(run, 10))
                out.append((17, r - 3))
        elif i > 0 and lens[i - 1] == v and run >= 3 and rng.random() < 0.8:
            r = rng.randint(3, min(run, 6))
            out.append((16, r - 3))
        else:
            r = 1
            out.append((v, 0))
        i += r
    assert expand_header(out) == list(lens)
    return out


def _random_blocks(rng):
    n_blocks, total = rng.randint(1, 4), rng.randint(1, 4096)
    alphabet = rng.sample(range(256), rng.randint(2, 24))
    cuts = sorted(rng.randint(0, total) for _ in range(n_blocks - 1)) + [total]
    blocks, o = [], 0
    for bi, end in enumerate(cuts):
        kind, final, room = rng.choice((dt.STORED, dt.FIXED, dt.DYNAMIC)), bi == n_blocks - 1, end - o
        if kind == dt.STORED:
            blocks.append(stored(bytes(rng.choice(alphabet) for _ in range(room)), final))
            o = end
            continue
        lone = kind == dt.DYNAMIC and rng.random() < 0.25                 # every match from one distance symbol
        lone_sym = rng.randint(0, dt.distance_symbol(o)) if lone and o else 0
        toks = []
        while o < end:
            if o and end - o >= 3 and rng.random() < 0.3:
                lo, hi = distance_range(lone_sym) if lone else (1, o)
                if lo <= o:
                    length = min(rng.randint(3, 258), end - o)
                    toks.append((length, rng.randint(lo, min(hi, o))))
                    o += length
                    continue
            toks.append(rng.choice(alphabet))
            o += 1
        if kind == dt.FIXED:
            blocks.append(fixed(toks, final))
            continue
        ll_hist, d_hist = dt.histograms(toks)
        ll_used, d_used = [s for s, f in enumerate(ll_hist) if f], [s for s, f in enumerate(d_hist) if f]
        hlit = rng.randint(max(ll_used) + 1, 286)
        ll = random_complete_lengths(rng, hlit, ll_used)
        if d_used:
            d = random_complete_lengths(rng, rng.randint(max(d_used) + 1, 30), d_used)
        else:
            d = rng.choice(([0], [1, 1], [0] * rng.randint(2, 30)))
        blocks.append(dynamic(toks, ll, d, final, header_symbols=random_runs(rng, ll + d)))
    return blocks


def random_members(seed, n):
    """([(name, body, text, marks)], summary) of n members of 1 .. 4096 bytes of text in 1 .. 4 blocks of random types:
    random tokens from a small alphabet (a match with probability 0.3, its distance uniform in 1 .. the text so far, its
    length uniform in 3 .. 258 within the room left), every dynamic block under a random complete code and a header of
    random run codes.  zlib has given every member's text.  summary: the run codes used, the longest code a token used,
    the blocks with a lone distance code, and the block types seen in first, middle and last place."""
    rng = random.Random(seed)
    out = []
    summary = {"run_codes": set(), "longest_code": 0, "lone_distance_blocks": 0, "first": set(), "middle": set(), "last": set()}
    for i in range(n):
        blocks = _random_blocks(rng)
        w = write(blocks)
        got, why = zlib_inflate(w.body)
        assert got == w.text and 1 <= len(w.text) <= 4096, (seed, i, why)
        out.append((f"random_{seed}_{i}", w.body, w.text, w.marks))
        summary["longest_code"] = max([summary["longest_code"]] + [bits for _, _, bits in w.widths])
        for bi, blk in enumerate(blocks):
            where = "first" if bi == 0 else "last" if bi == len(blocks) - 1 else "middle"
            summary[where].add(blk["type"])
            if len(blocks) == 1:
                summary["last"].add(blk["type"])
            if blk["type"] == dt.DYNAMIC:
                summary["run_codes"] |= {s for s, _ in blk["header"] if s >= 16}
                if sum(1 for x in blk["d"] if x) == 1 and any(isinstance(t, tuple) for t in blk["tokens"]):
                    summary["lone_distance_blocks"] += 1
    return out, summary


def check_summary(summary):
    """the seeded set must not thin out"""
    assert summary["run_codes"] == {16, 17, 18}, summary
    assert summary["longest_code"] == 15, summary
    assert summary["lone_distance_blocks"] >= 1, summary
    for where in ("first", "middle", "last"):
        assert summary[where] == {dt.STORED, dt.FIXED, dt.DYNAMIC}, (where, summary)


def random_files(C, seed=SEED, n=N_RANDOM, n_large=8):
    """{frame: (file, text, [(text offset, name, marks)])}: the random members as one multi-member file per frame; the
    large frame holds the first n_large of them, each behind the stored lead"""
    members, summary = random_members(seed, n)
    check_summary(summary)
    lead = large_lead(C)
    out = {}
    for frame in FRAMES:
        data, text, index = [], [], []
        at = 0
        for name, body, t, marks in members[:n_large] if frame == "bgzf64" else members:
            if frame == "bgzf64":
                body, t = write([stored(lead, False)]).body + body, lead + t
                marks = [(0, -1, ("stored", len(lead)))] + [(o + len(lead), b, tok) for o, b, tok in marks]
                assert zlib_inflate(body)[0] == t
            data.append(ic.wrap(body, t) if frame == "plain" else bc.frame(body, t))
            index.append((at, name, marks))
            text.append(t)
            at += len(t)
        out[frame] = (b"".join(data) + (b"" if frame == "plain" else bc.EOF), b"".join(text), index)
    return out


def where_in_file(got, text, index):
    """for a failure's message: the member of a random_files() file in which `got` leaves `text`, and the token there"""
    if got is None:
        return "not taken"
    n = next((i for i in range(min(len(got), len(text))) if got[i] != text[i]), min(len(got), len(text)))
    k = max(i for i, e in enumerate(index) if e[0] <= n or i == 0)
    at, name, marks = index[k]
    end = index[k + 1][0] if k + 1 < len(index) else len(text)
    return f"{name}: {first_difference(got[at:end], text[at:end], marks)}"


def dump(path, accepted_cases, refused_cases, frame, extra=()):
    """the cases of one container ("plain": what tools/inflate_host_check.cpp reads; else tools/bgzf_host_check.cpp's) in
    the record format of inflate_cases.dump / bgzf_cases.dump; extra: further accepted (name, file, text)"""
    plain = frame == "plain"
    ok = [(f"{c.name}-{c.frame}", c.data, c.text) for c in accepted_cases if (c.frame == "plain") == plain] + list(extra)
    bad = [(f"{r.name}-{r.frame}", r.data, r.member, r.reason) for r in refused_cases if (r.frame == "plain") == plain]
    return bc.dump(path, ok, bad)
