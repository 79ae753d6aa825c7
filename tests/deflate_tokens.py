"""A gzip / deflate reader that keeps the tokens, and the two match rules of the device gzip encoder as plain Python models
(csrc/pf_deflate.h: host_model_chunk; csrc/pf_deflate.hip: gz_encode_kernel).  Pure Python, no GPU: what the tests of
tests/test_deflate_host_model.py and tests/test_gpu_deflate.py compare the encoders' bytes with."""
import collections
import functools
import heapq
import zlib

STORED, FIXED, DYNAMIC = 0, 1, 2
MEMBER_HEAD = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
MAX_MATCH, HASH_BITS, MAX_BITS = 258, 12, 15
N_LL, N_D = 286, 30

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = tuple([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = tuple([5] * 30)


class BadStream(AssertionError):
    pass


def _need(cond, what):
    if not cond:
        raise BadStream(what)


def length_symbol(length):
    """RFC 1951 3.2.5: 3..258 -> 257..285"""
    if length == 258:
        return 285
    s = 0
    while s + 1 < 28 and LENGTH_BASE[s + 1] <= length:
        s += 1
    return 257 + s


def distance_symbol(dist):
    """1..32768 -> 0..29"""
    s = 0
    while s + 1 < 30 and DIST_BASE[s + 1] <= dist:
        s += 1
    return s


def length_range(sym):
    """the first and last length of a length symbol"""
    s = sym - 257
    return LENGTH_BASE[s], (258 if sym == 285 else LENGTH_BASE[s] + (1 << LENGTH_EXTRA[s]) - 1 - (1 if sym == 284 else 0))


def token_width(tok, ll_len, d_len):
    """the bits a token takes under the given code lengths"""
    if isinstance(tok, int):
        return ll_len[tok]
    ls, ds = length_symbol(tok[0]), distance_symbol(tok[1])
    return ll_len[ls] + LENGTH_EXTRA[ls - 257] + d_len[ds] + DIST_EXTRA[ds]


def histograms(tokens):
    """(literal/length, distance) frequencies of a token list, the end-of-block symbol counted once"""
    ll, d = [0] * N_LL, [0] * N_D
    for t in tokens:
        if isinstance(t, int):
            ll[t] += 1
        else:
            ll[length_symbol(t[0])] += 1
            d[distance_symbol(t[1])] += 1
    ll[256] = 1
    return ll, d


def huffman(hist):
    """(cost, depth) of a plain Huffman code of the used symbols of `hist`, by heap.  Ties go to the leaf before the
    inner node and to the older inner node, which is the order the encoder's two-queue builder merges in: the depth is
    that of the tree the encoder limits.  Fewer than two used symbols: one bit each, as a complete code needs."""
    heap = [(f, 0, s, 0) for s, f in enumerate(hist) if f]              # (weight, inner?, sequence, depth below)
    if len(heap) < 2:
        return sum(hist), 1
    heapq.heapify(heap)
    cost, seq = 0, 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        seq += 1
        heapq.heappush(heap, (a[0] + b[0], 1, seq, max(a[3], b[3]) + 1))
    return cost, heap[0][3]


def kraft(lengths):
    """the Kraft sum of the non-zero lengths, in units of 2^-15"""
    return sum(1 << (MAX_BITS - n) for n in lengths if n)


class _Bits:
    def __init__(self, raw, at):
        self.raw, self.byte, self.buf, self.cnt, self.start = raw, at, 0, 0, at

    def fill(self, n):
        while self.cnt < n:
            _need(self.byte < len(self.raw), "the stream ends inside a block")
            self.buf |= self.raw[self.byte] << self.cnt
            self.byte += 1
            self.cnt += 8

    def take(self, n):
        if self.cnt < n:
            self.fill(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def bitpos(self):
        return 8 * (self.byte - self.start) - self.cnt

    def align(self):
        self.byte -= self.cnt // 8          # the rest of the current byte goes, whole bytes read ahead come back
        self.buf, self.cnt = 0, 0


def _decoder(lengths):
    """a table from the next `width` bits of the stream to (symbol, length); None for a bit pattern no code has"""
    width = max(lengths)
    _need(width > 0, "a code without symbols")
    count = collections.Counter(n for n in lengths if n)
    code, nxt = 0, {}
    for b in range(1, width + 1):
        code = (code + count.get(b - 1, 0)) << 1
        nxt[b] = code
    _need(kraft(lengths) <= 1 << MAX_BITS, "an over-subscribed code")
    table = [None] * (1 << width)
    for s, n in enumerate(lengths):
        if n:
            c, nxt[n] = nxt[n], nxt[n] + 1
            r = int(format(c, f"0{n}b")[::-1], 2)
            table[r::1 << n] = [(s, n)] * (1 << (width - n))
    return table, width


def _symbol(bits, dec):
    table, width = dec
    if bits.cnt < width:
        bits.fill(width)                                    # (the member's tail of 8 bytes stands behind every block)
    e = table[bits.buf & ((1 << width) - 1)]
    _need(e is not None, "a bit pattern that is no code")
    bits.buf >>= e[1]
    bits.cnt -= e[1]
    return e[0]


def _dynamic_lengths(bits):
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    _need(hlit <= N_LL and hdist <= N_D, "HLIT / HDIST out of range")
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = bits.take(3)
    dec = _decoder(cl)
    lens = []
    while len(lens) < hlit + hdist:
        s = _symbol(bits, dec)
        if s < 16:
            lens.append(s)
        elif s == 16:
            _need(lens, "a repeat code with nothing before it")
            lens += [lens[-1]] * (3 + bits.take(2))
        elif s == 17:
            lens += [0] * (3 + bits.take(3))
        else:
            lens += [0] * (11 + bits.take(7))
    _need(len(lens) == hlit + hdist, "the code lengths run past HLIT + HDIST")
    return lens[:hlit] + [0] * (N_LL - hlit), lens[hlit:] + [0] * (N_D - hdist)


Member = collections.namedtuple("Member", "btype tokens ll_len d_len coded_bits first_token_bit text size")


def _member(raw, at):
    _need(raw[at:at + 10] == MEMBER_HEAD, f"member head {raw[at:at + 10].hex()}")
    bits = _Bits(raw, at + 10)
    _need(bits.take(1) == 1, "BFINAL is not set on the member's only block")
    btype = bits.take(2)
    _need(btype <= 2, "block type 3")
    out = bytearray()
    tokens, ll_len, d_len, first = None, None, None, None
    if btype == STORED:
        bits.align()
        ln, nln = bits.take(16), bits.take(16)
        _need(ln ^ nln == 0xFFFF, "NLEN is not LEN's complement")
        _need(bits.byte + ln <= len(raw), "a stored block runs past the stream")
        out += raw[bits.byte:bits.byte + ln]
        bits.byte += ln
        coded = 8 * (5 + ln)
    else:
        ll_len, d_len = (list(FIXED_LL[:N_LL]), list(FIXED_D)) if btype == FIXED else _dynamic_lengths(bits)
        _need(ll_len[256], "no end-of-block code")
        ll_dec = _decoder(ll_len if btype == DYNAMIC else FIXED_LL)
        d_dec = _decoder(d_len) if any(d_len) else None
        first = 80 + bits.bitpos()
        tokens = []
        while True:
            s = _symbol(bits, ll_dec)
            if s < 256:
                tokens.append(s)
                out.append(s)
            elif s == 256:
                break
            else:
                _need(s < N_LL, "length symbol 286 / 287")
                length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                _need(d_dec is not None, "a match in a block without distance codes")
                ds = _symbol(bits, d_dec)
                _need(ds < N_D, "distance symbol 30 / 31")
                dist = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                _need(dist <= len(out), f"a match {dist} back after {len(out)} bytes: it reaches before its chunk")
                tokens.append((length, dist))
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
        coded = bits.bitpos()
        bits.align()
    tail = bits.byte
    _need(tail + 8 <= len(raw), "the stream ends before the member's CRC32 and ISIZE")
    _need(int.from_bytes(raw[tail:tail + 4], "little") == zlib.crc32(out), "CRC32")
    _need(int.from_bytes(raw[tail + 4:tail + 8], "little") == len(out), "ISIZE")
    return Member(btype, tokens, ll_len, d_len, coded, first, bytes(out), tail + 8 - at)


def members(raw):
    """every member of a multi-member gzip stream as the encoder writes them: the fixed 10-byte head, one final block,
    CRC32, ISIZE.  Per member: block type, tokens (an int literal or a (length, distance) pair; None when stored), the
    286 + 30 code lengths of a dynamic block (the fixed ones of a fixed block), the coded bits from BFINAL to the
    end-of-block code, the bit offset of the first token in the member, the text, the member's size."""
    raw, out, at = bytes(raw), [], 0
    while at < len(raw):
        m = _member(raw, at)
        out.append(m)
        at += m.size
    return out


def token_offsets(m):
    """the bit offset of each token of a coded member from the member's first byte, from its coded bits: the tokens and
    the end-of-block code are the block's last bits"""
    widths = [token_width(t, m.ll_len, m.d_len) for t in m.tokens]
    at = 80 + m.coded_bits - m.ll_len[256] - sum(widths)
    _need(at == m.first_token_bit, "the tokens' widths do not add up to the coded bits")
    offs = []
    for w in widths:
        offs.append(at)
        at += w
    return offs, widths


def third_word_tokens(m):
    """the widths of the tokens put_bits writes into three 32-bit words: (offset & 31) + width > 64"""
    offs, widths = token_offsets(m)
    return [w for o, w in zip(offs, widths) if (o & 31) + w > 64]


# ---- the match rules
def hash4(w):
    return ((w * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def hashes(chunk):
    """hash4 of the four bytes at every position p with p + 3 < n"""
    return [hash4(int.from_bytes(chunk[p:p + 4], "little")) for p in range(len(chunk) - 3)]


def match_ok(length, dist):
    return length >= 4 or (length == 3 and dist <= 4096)


def _extend(chunk, c, p):
    maxl = min(MAX_MATCH, len(chunk) - p)
    if chunk[c:c + maxl] == chunk[p:p + maxl]:
        return maxl
    length = 0
    while chunk[c + length] == chunk[p + length]:
        length += 1
    return length


def _greedy(chunk, cands, literals_only):
    """cands[p]: the candidate position of p, or None.  A match that match_ok takes, or one literal, then the position
    behind it."""
    tokens, p, n = [], 0, len(chunk)
    while p < n:
        c = None if literals_only else cands[p]
        if c is not None:
            length = _extend(chunk, c, p)
            if match_ok(length, p - c):
                tokens.append((length, p - c))
                p += length
                continue
        tokens.append(chunk[p])
        p += 1
    return tokens


@functools.lru_cache(maxsize=512)
def parse_host(chunk, literals_only=False):
    """the host model's rule: one table, every position inserted (those a match covers too), the candidate of a position
    is the last position before it with its hash4, match_ok, greedy"""
    h = hashes(chunk)
    last, cands = {}, [None] * len(chunk)
    for p, x in enumerate(h):
        cands[p] = last.get(x)
        last[x] = p
    return _greedy(chunk, cands, literals_only)


@functools.lru_cache(maxsize=512)
def parse_device(chunk, literals_only=False):
    """the kernel's rule: the candidate of a hashed position p is the largest hashed q with its hash4 and
    q // 8 < p // 8; every hashed position is inserted, covered by a match or not; match_ok, greedy"""
    h = hashes(chunk)
    last, cands = {}, [None] * len(chunk)
    for g in range(0, len(h), 8):
        group = range(g, min(g + 8, len(h)))
        for p in group:
            cands[p] = last.get(h[p])
        for p in group:
            last[h[p]] = p
    return _greedy(chunk, cands, literals_only)
