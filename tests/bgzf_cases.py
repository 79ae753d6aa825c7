"""BGZF for the tests (tests/test_bgzf_host_model.py on the CPU, tests/test_gpu_bgzf.py on the GPU): a maker and a walker
written from the SAM specification, section 4.1, and RFC 1952 -- independent of the product's code --, the files the
decoder must take, and the files it must refuse.  A BGZF file is a series of gzip members of at most 65 536 bytes, each
with FLG = 4 and one extra subfield 'B' 'C' of two bytes that holds the member's size - 1, and of at most 65 536 bytes of
text; it ends with a fixed 28-byte member of no text.  zlib writes and reads the raw deflate streams; the hand-made
streams use tests/inflate_cases.py's bit writer."""
import gzip
import os
import random
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_cases as ic  # noqa: E402

MAX = 65536                 # of a member's bytes, and of its text's
BLOCK = 65280               # bgzip's text bytes per member
EOF = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


# ---- the maker
def frame(body, text, mtime=0, xfl=0, os_=255):
    """one member around a raw deflate stream"""
    size = 18 + len(body) + 8
    assert size <= MAX and len(text) <= MAX, (size, len(text))
    return (struct.pack("<4BIBB", 0x1F, 0x8B, 8, 4, mtime, xfl, os_) + struct.pack("<H2BHH", 6, ord("B"), ord("C"), 2, size - 1) + body
            + struct.pack("<II", zlib.crc32(text), len(text)))


def deflate(text, level, sync=False):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    if sync:
        a, b = len(text) // 3, 2 * len(text) // 3
        return (z.compress(text[:a]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[a:b]) + z.flush(zlib.Z_SYNC_FLUSH)
                + z.compress(text[b:]) + z.flush())
    return z.compress(text) + z.flush()


def member(text, level=6, sync=False):
    return frame(deflate(text, level, sync), text)


def make(text, level=6, block=BLOCK, marker=True, sync=False):
    """the file bgzip would write of `text`: members of `block` bytes of text each, then the end marker"""
    return b"".join(member(text[at:at + block], level, sync) for at in range(0, len(text), block)) + (EOF if marker else b"")


# ---- the walker
def walk(data, marker=True, mtime=0):
    """[(member's offset, its size, its text)] of a BGZF file, every byte of every frame checked: ID1 ID2 CM = 8 FLG = 4,
    MTIME, XLEN = 6, 'B' 'C' SLEN = 2, BSIZE = size - 1, the raw deflate stream ending exactly at the tail, CRC32 and ISIZE
    of the text it gives, ISIZE <= 65 536; with `marker` the last 28 bytes are the end-of-file member"""
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 18 + 8, f"member at {at}: {len(data) - at} bytes left"
        id1, id2, cm, flg, mt, xfl, os_ = struct.unpack_from("<4BIBB", data, at)
        assert (id1, id2, cm, flg) == (0x1F, 0x8B, 8, 4), f"member at {at}: head {data[at:at + 4].hex()}"
        assert mt == mtime, f"member at {at}: MTIME {mt}"
        xlen, si1, si2, slen, bsize = struct.unpack_from("<H2BHH", data, at + 10)
        assert (xlen, si1, si2, slen) == (6, 0x42, 0x43, 2), f"member at {at}: extra field {data[at + 10:at + 18].hex()}"
        size = bsize + 1
        assert 18 + 8 <= size <= len(data) - at, f"member at {at}: BSIZE {bsize}"
        d = zlib.decompressobj(-15)
        text = d.decompress(data[at + 18:at + size - 8])
        assert d.eof and not d.unused_data and not d.unconsumed_tail, f"member at {at}: the stream does not end at the tail"
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert isize == len(text) <= MAX and crc == zlib.crc32(text), f"member at {at}: tail"
        out.append((at, size, text))
        at += size
    if marker:
        assert data[-28:] == EOF and out and out[-1][1] == 28, "no end-of-file member"
    return out


def walked_text(data, marker=True):
    return b"".join(t for _, _, t in walk(data, marker))


# ---- texts
def tsv_text(n, seed=1):
    """n bytes of rows like kmers_to_hashes.tsv's: a k-mer, a tab, a 24-character hash"""
    rng = random.Random(seed)
    hashes = ["".join(rng.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/") for _ in range(22)) + "=="
              for _ in range(40)]
    rows, size = [], 0
    while size < n:
        row = "".join(rng.choice("ACGT") for _ in range(31)) + "\t" + rng.choice(hashes) + "\n"
        rows.append(row)
        size += len(row)
    return "".join(rows).encode()[:n]


def noise(n, seed=2):
    return random.Random(seed).randbytes(n)


# ---- hand-made members: fixed codes (RFC 1951 3.2.6) behind stored blocks
def stored_block(data, final=False):
    assert len(data) <= 65535
    return ic.Bits().put(1 if final else 0, 1).put(0, 2).align().put(len(data), 16).put(len(data) ^ 0xFFFF, 16).bytes() + data


def fixed_match_block(matches):
    """one final fixed-code block of matches (length 3 or 258, distance 1 or 32 768) and nothing else"""
    b = ic.Bits().put(1, 1).put(1, 2)
    for length, dist in matches:
        b.code({3: 1, 258: 0xC5}[length], {3: 7, 258: 8}[length])            # length symbols 257 and 285
        if dist == 1:
            b.code(0, 5)
        else:
            assert dist == 32768
            b.code(29, 5).put(32768 - 24577, 13)                              # distance symbol 29, 13 extra bits
    return b.code(0, 7).bytes()                                               # end of block


def flushed_blocks(data):
    """`data` as non-final blocks by zlib that end at a byte boundary (a sync flush): a lead too long to be stored"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    return z.compress(data) + z.flush(zlib.Z_SYNC_FLUSH)


def copy(text, length, dist):
    out = bytearray(text)
    for _ in range(length):
        out.append(out[-dist])
    return bytes(out)


def hand_made():
    """[(name, member, text)]: matches only a window of more than 32 KiB has -- offsets above 32 767, a distance of 32 768
    whose source is the window's first half, the member's very last byte"""
    out = []
    base = tsv_text(65536, seed=5)
    for name, lead, length, dist in (("match_258_at_32768_from_byte_0", 32768, 258, 32768),
                                     ("run_258_across_32768", 32768 - 100, 258, 1),
                                     ("match_3_ends_at_65536", 65533, 3, 1),
                                     ("match_258_at_65278_ends_at_65536", 65278, 258, 32768)):
        text = copy(base[:lead], length, dist)
        blocks = stored_block(base[:lead]) if lead < 65000 else flushed_blocks(base[:lead])
        out.append((name, frame(blocks + fixed_match_block([(length, dist)]), text), text))
    return out


def accepted(C):
    """[(name, file, text)], each checked by the walker and by gzip before it is used"""
    tsv = tsv_text(300000)
    out = [("empty_file_marker_only", EOF, b"")]
    for n in (1, C - 1, C, C + 1, 65279, 65280, 65535, 65536):
        out.append((f"one_member_{n}", make(tsv[:n], 6, block=MAX), tsv[:n]))
    for level in (1, 6, 9):
        out.append((f"tsv_300k_level{level}", make(tsv, level), tsv))
    out.append(("stored_65280_blocks", make(noise(3 * BLOCK), 0), noise(3 * BLOCK)))
    out.append(("sync_flush_inside", make(tsv[:2 * BLOCK + 77], 6, sync=True), tsv[:2 * BLOCK + 77]))
    out.append(("no_end_marker", make(tsv[:100000], 6, marker=False), tsv[:100000]))
    out.append(("stored_full_member", frame(stored_block(noise(65000, 3), True), noise(65000, 3)) + EOF, noise(65000, 3)))
    out += [(name, m + EOF, text) for name, m, text in hand_made()]
    for name, data, text in out:
        assert gzip.decompress(data) == text, name
        assert walked_text(data, marker=name != "no_end_marker") == text, name
    return out


def refused(C):
    """[(name, file, the member refused, the check's name)]; zlib takes the first four as gzip files all the same"""
    tsv = tsv_text(3 * BLOCK)
    good = make(tsv, 6)
    ms = walk(good)
    m0, m1 = good[:ms[0][1]], good[ms[1][0]:ms[1][0] + ms[1][1]]
    body, t0 = m0[18:-8], ms[0][2]
    out = [("bsize_past_the_end", good[:ms[2][0] + ms[2][1] - 5], 2, "truncated")]
    out.append(("bsize_20", m0 + m1[:16] + struct.pack("<H", 20) + m1[18:], 1, "bad header"))
    two = m0[:10] + struct.pack("<H2BHH2BHH", 12, 0x42, 0x43, 2, len(m0) + 6 - 1, ord("X"), ord("Y"), 2, 7) + m0[18:]
    assert gzip.decompress(two) == t0
    out.append(("xlen_12_two_subfields", two + EOF, 0, "bad header"))
    other = m0[:12] + b"XY" + m0[14:]
    assert gzip.decompress(other) == t0
    out.append(("flg_4_without_bc", other + EOF, 0, "bad header"))
    plain = ic.wrap(body, t0)
    assert gzip.decompress(m0 + plain + m1 + EOF) == t0 + t0 + ms[1][2]
    out.append(("plain_member_in_the_chain", m0 + plain + m1 + EOF, 1, "bad header"))
    out.append(("isize_65537", m0 + m1[:-4] + struct.pack("<I", 65537) + EOF, 1, "too large"))
    out.append(("isize_one_more", m0[:-4] + struct.pack("<I", len(t0) + 1) + EOF, 0, "less text than ISIZE"))
    out.append(("isize_one_less", m0[:-4] + struct.pack("<I", len(t0) - 1) + EOF, 0, "more text than ISIZE"))
    out.append(("flipped_crc", m0 + m1[:-8] + bytes([m1[-8] ^ 1]) + m1[-7:] + EOF, 1, "CRC32 differs"))
    half = body[:len(body) // 2]
    out.append(("payload_cut_tail_kept", m0[:16] + struct.pack("<H", 18 + len(half) + 8 - 1) + half + m0[-8:] + EOF, 0, "truncated"))
    lead = tsv[:32767]
    # (the tail's text is never compared: the match is refused where it is read)
    out.append(("distance_before_byte_0", frame(stored_block(lead) + fixed_match_block([(258, 32768)]), lead + b"?" * 258) + EOF, 0,
                "distance before the start"))
    return out


def dump(path, accepted_items, refused_items):
    """records of taken (u32), name length (u32), name, file length (u64), file, text length (u64), text, little-endian:
    what tools/bgzf_host_check.cpp reads"""
    with open(path, "wb") as fh:
        for taken, items in ((1, accepted_items), (0, [(n, d, b"") for n, d, _, _ in refused_items])):
            for name, data, text in items:
                fh.write(struct.pack("<II", taken, len(name)) + name.encode())
                fh.write(struct.pack("<Q", len(data)) + data + struct.pack("<Q", len(text)) + text)
    return len(accepted_items), len(refused_items)
