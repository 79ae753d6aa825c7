"""Inputs of the device gunzip tests (tests/test_inflate_host_model.py on the CPU, tests/test_gpu_inflate.py on the GPU):
gzip files made of small members, from three independent encoders over the texts of tests/deflate_cases.py, member
layouts, and members that must be refused.  zlib is the reference: every accepted input is inflated by gzip.decompress
and must give its text before it is used.  C is pf_gzip_device_chunk_bytes()."""
import gzip
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_tokens as dt  # noqa: E402

HEAD = dt.MEMBER_HEAD


def slot_bytes(C):
    """the largest member the decoder takes (csrc/pf_deflate.h SLOT_BYTES)"""
    return (C + C // 8 + 256 + 15) & ~15


def tail(text):
    return zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little")


def wrap(payload, text):
    return HEAD + payload + tail(text)


def zlib_member(text, level, sync=False):
    """raw deflate by zlib in the plain 10-byte header with a computed tail; sync: Z_SYNC_FLUSH twice inside the text
    (non-final blocks, empty stored blocks mid-stream, byte realignment, matches across a block boundary)"""
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    if sync:
        a, b = len(text) // 3, 2 * len(text) // 3
        body = (z.compress(text[:a]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(text[a:b]) + z.flush(zlib.Z_SYNC_FLUSH)
                + z.compress(text[b:]) + z.flush())
    else:
        body = z.compress(text) + z.flush()
    return wrap(body, text)


def zlib_members(text, C, level, sync=False):
    return b"".join(zlib_member(text[at:at + C], level, sync) for at in range(0, len(text), C))


def checked(name, members, text, C):
    """the input as (name, members, text), after the reference has agreed"""
    assert (gzip.decompress(members) if members else b"") == text, name
    return name, members, text


def texts(C):
    """the distinct texts of deflate_cases.cases(C)"""
    seen = {}
    for name, data, _ in dc.cases(C):
        seen.setdefault(data, name)
    return [(name, data) for data, name in seen.items()]


def zlib_inputs(C):
    """{group: [(name, members, text)]}: every text per C-byte chunk at levels 1, 6 and 9, and with two sync flushes"""
    groups = {}
    for what, level, sync in (("zlib1", 1, False), ("zlib6", 6, False), ("zlib9", 9, False), ("zlib_sync", 6, True)):
        groups[what] = [checked(f"{what}-{name}", zlib_members(data, C, level, sync), data, C) for name, data in texts(C)]
    return groups


def encoder_inputs(C, encode):
    """[(name, members, text)] of encode(data, flags) -> members (pf_gzip_host_model or pf_gzip_device) under every flag
    set of every case"""
    return [checked(f"enc-{name}", encode(data, flags), data, C) for name, data, flags in dc.flat_cases(C)]


def layout_inputs(C, encode):
    """member layouts: counts that are no multiple of anything a launch rounds to, short members between full ones, a
    member of zero bytes, one chunk of every kind in a row"""
    rows = dc.real_shapes(C)["kmers_to_hashes"]
    out = []
    for k in (1, 3, 5, 17):
        piece, text = C // 4, rows[:k * (C // 4) - 3]
        members = b"".join(zlib_member(text[at:at + piece], 6) for at in range(0, len(text), piece))
        assert members.count(HEAD) >= k and len(text) > (k - 1) * piece
        out.append(checked(f"zlib_{k}_members", members, text, C))
    parts = [rows[:C + 1], rows[C + 1:C + 2], rows[C + 2:3 * C + 5]]
    out.append(checked("three_encode_calls", b"".join(encode(p, 0) for p in parts), b"".join(parts), C))
    out.append(checked("zlib_empty_member", zlib_member(b"", 6), b"", C))
    out.append(checked("zlib_empty_member_between", zlib_member(rows[:100], 6) + zlib_member(b"", 9) + zlib_member(rows[100:300], 1),
                       rows[:300], C))
    kinds = b"".join(text for _, text, _ in dc.chunk_kinds(C))
    out.append(checked("chunk_kinds_encoder", encode(kinds, 0), kinds, C))
    out.append(checked("chunk_kinds_zlib", zlib_members(kinds, C, 9), kinds, C))
    return out


# ---- members that must be refused, built by hand or by damaging a good one
class Bits:
    """a deflate bit stream under construction: values least significant bit first, Huffman codes from their top bit"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):
        return self.put(int(format(code, f"0{nbits}b")[::-1], 2), nbits) if nbits else self

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951 3.2.2"""
    codes, code = {}, 0
    for bits in range(1, 16):
        for sym, n in enumerate(lengths):
            if n == bits:
                codes[sym] = (code, bits)
                code += 1
        code <<= 1
    return codes


CL_LENGTHS = [4 if (s == 0 or 3 <= s <= 14) else 5 for s in range(19)]     # a complete code over all 19 symbols
CL_CODES = canonical(CL_LENGTHS)


def dynamic_head(ll_lens, d_lens, first=()):
    """BFINAL = 1, BTYPE = 2 and the header of a block with these code lengths, written one by one; `first`:
    code-length symbols (symbol, extra value, extra bits) put in front of them, in place of as many lengths"""
    b = Bits().put(1, 1).put(2, 2).put(len(ll_lens) - 257, 5).put(len(d_lens) - 1, 5).put(19 - 4, 4)
    for s in dt.CL_ORDER:
        b.put(CL_LENGTHS[s], 3)
    for sym, extra, nbits in first:
        b.code(*CL_CODES[sym]).put(extra, nbits)
    for n in (list(ll_lens) + list(d_lens))[len(first):]:
        b.code(*CL_CODES[n])
    return b


def fixed_literal(b, byte):
    return b.code(0x30 + byte, 8) if byte < 144 else b.code(0x190 + byte - 144, 9)


def rejected(C, encode):
    """[(name, members)]: each must come back not taken"""
    text = dc.real_shapes(C)["kmers_to_hashes"][:3000]
    good = encode(text, dc.DYNAMIC_ONLY)
    assert gzip.decompress(good) == text and good[10] & 7 == 5            # one final dynamic block
    body = good[10:-8]
    out = [("cut_mid_payload", good[:len(good) // 2]),
           ("payload_cut_tail_kept", HEAD + body[:len(body) // 2] + good[-8:]),
           ("cut_mid_tail", good[:-3])]
    flipped = bytearray(good)
    flipped[10 + len(body) // 2] ^= 0x10
    out.append(("flipped_bit", bytes(flipped)))
    out.append(("wrong_crc", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:]))
    out.append(("isize_one_less", good[:-4] + (len(text) - 1).to_bytes(4, "little")))
    out.append(("isize_one_more", good[:-4] + (len(text) + 1).to_bytes(4, "little")))
    full = encode(b"a" * C, 0)
    out.append(("isize_chunk_plus_1", full[:-4] + (C + 1).to_bytes(4, "little")))
    # fixed codes; the first token is the match (3, 1): length symbol 257, distance symbol 0
    b = Bits().put(1, 1).put(1, 2).code(1, 7).code(0, 5).code(0, 7)
    out.append(("match_before_start", wrap(b.bytes(), b"aaa")))
    # three literal/length symbols of one bit
    ll = [0] * 257
    ll[97] = ll[98] = ll[256] = 1
    out.append(("oversubscribed_literal_code", wrap(dynamic_head(ll, [1, 1]).put(0, 8).bytes(), b"a")))
    # a complete literal/length code, two distance symbols of two bits
    ll = [0] * 257
    ll[97] = ll[256] = 1
    out.append(("incomplete_distance_code", wrap(dynamic_head(ll, [2, 2]).code(0, 1).code(1, 1).bytes(), b"a")))
    # the very same block with a complete distance code is taken: the refusal above is the code's
    ok = wrap(dynamic_head(ll, [1, 1]).code(0, 1).code(1, 1).bytes(), b"a")
    assert gzip.decompress(ok) == b"a"
    out.append(("repeat_without_a_length", wrap(dynamic_head(ll, [1, 1], first=[(16, 0, 2)] * 1).code(0, 1).code(1, 1).bytes(), b"a")))
    out.append(("stored_len_nlen", wrap(Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xFFFD, 16).bytes() + b"abc", b"abc")))
    b = Bits().put(1, 1).put(1, 2)
    for c in b"abc":
        fixed_literal(b, c)
    out.append(("no_end_of_block", wrap(b.bytes(), b"abc")))
    b = Bits().put(1, 1).put(1, 2)
    for c in b"abcd":
        fixed_literal(b, c)
    out.append(("more_than_isize", wrap(b.code(0, 7).bytes(), b"abc")))
    out.append(("block_type_3", wrap(Bits().put(1, 1).put(3, 2).bytes(), b"")))
    # a stored block whose text holds the signature behind eight bytes that read as a tail: a false candidate
    inner = b"a" * 30 + tail(b"0123456789") + HEAD + b"b" * 40
    stored = wrap(Bits().put(1, 1).put(0, 2).align().put(len(inner), 16).put(len(inner) ^ 0xFFFF, 16).bytes() + inner, inner)
    assert gzip.decompress(stored) == inner
    out.append(("signature_in_stored_text", stored))
    out.append(("bad_member_between_good_ones", good + out[4][1] + good))
    for name, raw in out:
        assert len(raw) <= 3 * slot_bytes(C), name
    return out, ok


def dump(path, C, encode, accepted=None):
    """every accepted (made here unless given) and every rejected input as records of taken (u32), name length (u32), name, members length
    (u64), members, text length (u64), text, little-endian: what tools/inflate_host_check.cpp reads"""
    if accepted is None:
        accepted = encoder_inputs(C, encode) + layout_inputs(C, encode) + [i for g in zlib_inputs(C).values() for i in g]
    accepted = list(accepted)
    refused, ok = rejected(C, encode)
    accepted.append(("hand_made_dynamic", ok, b"a"))
    with open(path, "wb") as fh:
        for taken, items in ((1, accepted), (0, [(n, m, b"") for n, m in refused])):
            for name, members, text in items:
                fh.write(taken.to_bytes(4, "little") + len(name).to_bytes(4, "little") + name.encode())
                fh.write(len(members).to_bytes(8, "little") + members + len(text).to_bytes(8, "little") + text)
    return len(accepted), len(refused)
