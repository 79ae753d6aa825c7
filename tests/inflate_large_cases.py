"""Inputs for the large-member gunzip route (tests/test_inflate_large_host.py on the CPU, tests/test_gpu_inflate_large.py on
the GPU): gzip members as other writers make them -- one member a file, any RFC 1952 head, many deflate blocks -- small
enough that with piece_bytes of 64 to 512 a member of 20 to 80 KiB of text has tens of pieces.  zlib is the reference:
every accepted file gives its text under gzip.decompress, every refused one is refused by it, before it is used.  The
hand-written streams go from tokens to bits through tests/inflate_edges.py's writer.  Pure Python, no GPU."""
import collections
import gzip
import os
import random
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgzf_cases as bc  # noqa: E402
import inflate_edges as ie  # noqa: E402

WINDOW = 32768
MANY = 3000                              # members of the case that has more of them than a call takes
PIECES = (64, 200, 512)                  # piece_bytes every case runs with
DEFAULT_TOO = ("zlib6_mem1", "handmade_chain", "stored_stream_inside")      # and these at the default (0: 32 KiB) as well

Case = collections.namedtuple("Case", "name data text pieces")
Refused = collections.namedtuple("Refused", "name data pieces host_text")      # host_text: what gzip gives, None where it raises

FEXTRA, FNAME, FCOMMENT, FHCRC = 4, 8, 16, 2


def member(body, text, flg=0, mtime=0, extra=b"xy\x02\x00ab", name=b"kmers.tsv", comment=b"a comment", isize=None, crc=None):
    """a gzip member of the raw deflate stream `body` under a head with the fields `flg` asks for"""
    head = bytes([0x1F, 0x8B, 8, flg]) + struct.pack("<IBB", mtime, 0, 255)
    if flg & FEXTRA:
        head += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        head += name + b"\0"
    if flg & FCOMMENT:
        head += comment + b"\0"
    if flg & FHCRC:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) if isize is None else isize) & 0xFFFFFFFF)


def deflate(text, level=6, mem=1, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=None):
    """the raw deflate stream of `text`; sync_every: a Z_SYNC_FLUSH behind every so many bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if not sync_every:
        return c.compress(text) + c.flush()
    parts = []
    for at in range(0, len(text), sync_every):
        parts += [c.compress(text[at:at + sync_every]), c.flush(zlib.Z_SYNC_FLUSH)]
    return b"".join(parts) + c.flush()


def tsv(n, seed):
    return bc.tsv_text(n, seed=seed)


# ---- the hand-written stream: five dynamic blocks, each a piece of its own at piece_bytes = 64 (a block's header alone
# is over 150 bytes)
def handmade_blocks(seed=11):
    rng = random.Random(seed)
    lits = lambda n: [rng.randrange(256) for _ in range(n)]                       # noqa: E731
    n0 = WINDOW + 700
    b0, have = lits(400), 400
    while have + 258 <= n0:                                  # text in front: over 32 KiB, so a distance of 32 768 exists
        b0.append((258, rng.randrange(1, min(have, WINDOW) + 1)))
        have += 258
    b0 += lits(n0 - have)
    # a match at distance 32 768 across the piece boundary; an overlapped copy (distance 3 < length 200) whose source is
    # what that match gave: markers, in the marker pass; length 258 ending exactly at the piece's end
    b1 = [(258, WINDOW), 7, (3, WINDOW), (200, 3)] + lits(50) + [(258, 1000)]
    n1 = 258 + 1 + 3 + 200 + 50 + 258
    b2 = lits(100) + [(258, rng.randrange(5000, 20000)) for _ in range(11)] + lits(62)
    b3 = lits(100) + [(258, rng.randrange(5000, 20000)) for _ in range(11)] + lits(62)
    n2 = n3 = 100 + 11 * 258 + 62
    assert n2 == 3000
    # matches that reach back through one, two and three pieces of less than 32 KiB of text each
    b4 = [(100, 3500), (100, n3 + n2 + 300 + 100), (100, n3 + n2 + n1 + 400 + 200), 9, (258, WINDOW), (258, 260)] + lits(20) + [(258, 5)]
    blocks = [ie.dynamic(t, ie.FULL_LL, ie.FULL_D, i == 4) for i, t in enumerate((b0, b1, b2, b3, b4))]
    w = ie.write(blocks)
    assert len(w.text) > n0 + n1 + n2 + n3 and ie.zlib_inflate(w.body)[0] == w.text
    return w


def stored_stream_inside(seed=5):
    """a stored block whose payload is a complete other deflate stream: real block headers where no block starts"""
    inner = deflate(tsv(24000, seed), 6, 1)
    assert 2000 < len(inner) < 60000
    lead, trail = list(tsv(3000, seed + 1)), list(tsv(3000, seed + 2))
    w = ie.write([ie.dynamic(lead, ie.FULL_LL, ie.FULL_D, False), ie.stored(inner, False), ie.dynamic(trail + [(258, 4000)], ie.FULL_LL, ie.FULL_D, True)])
    assert ie.zlib_inflate(w.body)[0] == w.text and inner in w.text
    return w


def small_members(text, encode):
    """`text` as this project's own device encoder writes it: members of at most 32 KiB of text"""
    return encode(text, 0)


def accepted(encode=None):
    """the files that must be taken; encode(text, flags): the device encoder's host model, for the case that needs small
    members (left out without it)"""
    out = []

    def add(name, data, text, pieces=None):
        assert gzip.decompress(data) == text, name
        out.append(Case(name, data, text, pieces or PIECES + ((0,) if name in DEFAULT_TOO else ())))

    text = tsv(60000, 3)
    for level in (1, 6, 9):
        add(f"zlib{level}_mem1", member(deflate(text, level, 1), text), text)
    add("sync_flush", member(deflate(text, 6, 1, sync_every=3000), text), text)
    add("fixed_only", member(deflate(tsv(20000, 4), 6, 8, zlib.Z_FIXED), tsv(20000, 4)), tsv(20000, 4))
    add("stored_only", member(deflate(tsv(80000, 6), 0), tsv(80000, 6)), tsv(80000, 6))
    w = handmade_blocks()
    add("handmade_chain", member(w.body, w.text), w.text)
    w = stored_stream_inside()
    add("stored_stream_inside", member(w.body, w.text), w.text)
    small = tsv(20000, 7)
    body = deflate(small, 6, 1)
    for name, flg in (("fextra", FEXTRA), ("fname", FNAME), ("fcomment", FCOMMENT), ("fhcrc", FHCRC), ("all_fields", FEXTRA | FNAME | FCOMMENT | FHCRC)):
        add("head_" + name, member(body, small, flg, mtime=1700000000), small)
    other = tsv(25000, 8)
    add("two_members_two_heads", member(body, small, FNAME, mtime=12345) + member(deflate(other, 9, 1), other, FCOMMENT | FHCRC), small + other)
    add("empty_member", member(deflate(b""), b""), b"")
    # large members in a row under one signature, as --compress writes them: decoded side by side, also behind a member that
    # was open when its call began
    row = [tsv(40000, 20 + i) for i in range(4)]          # (over the small-member kernels' 32 KiB of text)
    add("large_members_in_a_row", b"".join(member(deflate(t, 6, 1), t) for t in row), b"".join(row))
    # more members under one signature than a call has starts (2 048): their payloads are starts only as far as there is room
    rows = [b"r%d\n" % i for i in range(MANY)]
    add("many_tiny_members", b"".join(member(deflate(r), r, FNAME, name=b"t") for r in rows), b"".join(rows), (64, 512))
    if encode is not None:
        a, c = tsv(40000, 9), tsv(33000, 10)
        add("large_between_small", small_members(a, encode) + member(deflate(text, 6, 1), text) + small_members(c, encode), a + text + c)
    return out


def refused():
    """files that must not be taken: gzip.decompress raises for each, but for the reserved FLG bit, which Python's gzip does
    not look at"""
    text = tsv(60000, 3)
    body = deflate(text, 6, 1)
    good = member(body, text)
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10
    w = ie.write([ie.dynamic(list(b"abc") + [("far", 5, 4)] + list(b"xyz"), ie.FULL_LL, ie.FULL_D, True)])
    out = [Refused("reserved_flg_bit", member(body, text, 0x20), PIECES, text),
           Refused("flipped_bit", bytes(flipped), PIECES, None),
           Refused("cut_in_last_block", good[:-8 - 5], PIECES, None),
           Refused("cut_in_tail", good[:-3], PIECES, None),
           Refused("match_before_start", member(w.body, b"abc" + b"?" * 5 + b"xyz"), PIECES, None),
           Refused("isize_one_more", member(body, text, isize=len(text) + 1), PIECES, None),
           Refused("isize_one_less", member(body, text, isize=len(text) - 1), PIECES, None),
           Refused("cm_not_8", good[:2] + b"\x07" + good[3:], PIECES, None)]
    for r in out:
        try:
            got = gzip.decompress(r.data)
        except (OSError, EOFError, zlib.error):
            got = None
        assert got == r.host_text, r.name
    return out


def dump(path, cases, bad):
    """the cases as tools/inflate_large_host_check.cpp reads them, one record per (case, piece_bytes); -> (accepted, refused) records"""
    n_ok = n_bad = 0
    with open(path, "wb") as fh:
        for taken, items in ((1, cases), (0, bad)):
            for c in items:
                for piece in c.pieces:
                    text = c.text if taken else b""
                    name = c.name.encode()
                    fh.write(struct.pack("<III", taken, piece, len(name)) + name + struct.pack("<Q", len(c.data)) + c.data +
                             struct.pack("<Q", len(text)) + text)
                    n_ok, n_bad = n_ok + taken, n_bad + 1 - taken
    return n_ok, n_bad
