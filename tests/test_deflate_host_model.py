"""The gzip container and deflate coder of the device encoder, run by its serial host model (pf_gzip_host_model: the same
host+device format functions as the kernel, csrc/pf_deflate.h) on the cases of tests/deflate_cases.py; the .gz writer that
takes host text and ready members; the --gpu-compress option.  No GPU."""
import ctypes as C
import functools
import gzip
import os
import random
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_tokens as dt  # noqa: E402

from panfeed_amd import _lib, cli  # noqa: E402
from panfeed_amd.engine import GzipMembers  # noqa: E402
from panfeed_amd.output import MemberGzipWriter, write_text  # noqa: E402


def host_model(data, flags):
    L = _lib.load()
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), flags, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def test_chunk_size_and_flags():
    assert 8 << 10 <= chunk_bytes() <= 64 << 10
    assert (_lib.GZ_FIXED_ONLY, _lib.GZ_DYNAMIC_ONLY, _lib.GZ_LITERALS_ONLY) == (dc.FIXED_ONLY, dc.DYNAMIC_ONLY, dc.LITERALS_ONLY)


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        flat = dc.flat_cases(chunk_bytes())
        metafunc.parametrize("case", flat, ids=[c[0] for c in flat])
    if "named" in metafunc.fixturenames:
        named = list(dc.cases(chunk_bytes()))
        metafunc.parametrize("named", named, ids=[c[0] for c in named])


def test_host_model_decodes_to_the_input(case):
    name, data, flags = case
    C_ = chunk_bytes()
    members = host_model(data, flags)
    dc.check_members(data, members, C_)
    if name.startswith("incompressible"):
        assert len(members) <= dc.incompressible_cap(len(data), C_)


# ---- the reader the token assertions rest on
def _as_member(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = z.compress(text) + z.flush()
    return dt.MEMBER_HEAD + body + zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little")


def test_reader_takes_what_zlib_writes():
    """all of RFC 1951, not only what this encoder emits: the code-length symbols 16 / 17 / 18, HLIT and HDIST below
    their largest values, stored and fixed blocks, members in a row"""
    rng = random.Random(5)
    words = [rng.randbytes(rng.randrange(3, 9)) for _ in range(40)]
    prose = b" ".join(rng.choice(words) for _ in range(3000))
    plain = zlib.Z_DEFAULT_STRATEGY
    texts = [(prose, 9, plain), (prose[:20], 9, zlib.Z_FIXED), (rng.randbytes(3000), 0, plain),
             (b"ab" * 5000 + bytes(range(256)), 6, plain), (prose, 1, zlib.Z_HUFFMAN_ONLY)]
    ms = dt.members(b"".join(_as_member(*t) for t in texts))
    assert [m.text for m in ms] == [t[0] for t in texts]
    assert [m.btype for m in ms] == [dt.DYNAMIC, dt.FIXED, dt.STORED, dt.FIXED, dt.DYNAMIC]
    assert any(0 in m.ll_len[257:] for m in ms if m.btype == dt.DYNAMIC)
    for m, t in zip(ms, texts):
        assert m.size == len(_as_member(*t))
        if m.tokens is not None:
            assert sum(dt.token_offsets(m)[1]) + m.ll_len[256] + m.first_token_bit - 80 == m.coded_bits
            assert sum(1 if isinstance(k, int) else k[0] for k in m.tokens) == len(m.text)
    assert all(isinstance(k, int) for k in ms[4].tokens) and any(not isinstance(k, int) for k in ms[0].tokens)


def test_reader_refuses_a_damaged_member():
    good = host_model(b"the row before, the row before, the row before\n", dc.DYNAMIC_ONLY)
    stored = host_model(random.Random(2).randbytes(600), 0)
    assert dt.members(good)[0].btype == dt.DYNAMIC and dt.members(stored)[0].btype == dt.STORED

    def flipped(raw, at, bit=1):
        b = bytearray(raw)
        b[at] ^= bit
        return bytes(b)
    for what, raw in (("head", flipped(good, 9)), ("BFINAL", flipped(good, 10)), ("CRC32", flipped(good, len(good) - 8)),
                      ("ISIZE", flipped(good, len(good) - 1)), ("NLEN", flipped(stored, 13)), ("cut", good[:-3])):
        with pytest.raises(dt.BadStream):
            dt.members(raw)
            pytest.fail(f"a wrong {what} was accepted")
    # a match that reaches before its member's text: "abcd" and then (4, 5), in a fixed block
    bits, n = 0, 0
    literals = [(int(format(0x30 + c, "08b")[::-1], 2), 8) for c in b"abcd"]
    match = [(int("0000010"[::-1], 2), 7), (int("00100"[::-1], 2), 5), (0, 1)]        # length 4; distance symbol 4, extra 0
    for v, nb in [(1, 1), (1, 2)] + literals + match + [(0, 7)]:
        bits |= v << n
        n += nb
    with pytest.raises(dt.BadStream, match="before its chunk"):
        dt.members(dt.MEMBER_HEAD + bits.to_bytes((n + 7) // 8, "little") + bytes(8))


def test_symbol_helpers_are_rfc_1951():
    assert [dt.length_symbol(L) for L in (3, 4, 10, 11, 12, 13, 18, 19, 257, 258)] == [257, 258, 264, 265, 265, 266, 268, 269,
                                                                                       284, 285]
    assert [dt.distance_symbol(D) for D in (1, 4, 5, 6, 7, 8, 9, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 5, 6, 28, 29, 29]
    assert dt.length_range(284) == (227, 257) and dt.length_range(285) == (258, 258) and dt.length_range(265) == (11, 12)
    assert dt.huffman([5, 0, 1, 1, 2]) == (15, 3) and dt.huffman([0, 7]) == (7, 1)


# ---- the cases do what they are built for, under both match rules
RULES = (dt.parse_host, dt.parse_device)


def _matches(tokens):
    return [t for t in tokens if not isinstance(t, int)]


def test_no_candidate_gives_a_three_byte_match():
    """two words that differ only in their top byte never share a hash4 bucket (the multiplier is odd, so the difference
    d << 24 times it keeps a non-zero top byte): a candidate always agrees in 0, 1, 2 or at least 4 bytes"""
    for d in range(1, 256):
        assert ((((d << 24) * 2654435761) & 0xFFFFFFFF) >> 20) % (1 << 12) != 0
    rng = random.Random(1)
    for _ in range(2000):
        w = rng.getrandbits(32)
        assert dt.hash4(w) != dt.hash4(w ^ (rng.randrange(1, 256) << 24))


def test_length_edges_are_every_class_boundary_and_give_one_match():
    assert set(dc.LENGTH_EDGES) == {L for s in range(258, 286) for L in dt.length_range(s)} and 3 not in dc.LENGTH_EDGES
    assert {dt.length_symbol(L) for L in dc.LENGTH_EDGES} == set(range(258, 286))
    for L in dc.LENGTH_EDGES:
        for rule in RULES:
            assert _matches(rule(dc.length_edge(L))) == [(L, 301)], (L, rule.__name__)


def test_distance_edges_end_with_a_match_at_their_distance():
    C_ = chunk_bytes()
    edges = [D for D in dc.DISTANCE_EDGES + dc.FAR_DISTANCE_EDGES if D + 8 <= C_]
    assert {dt.distance_symbol(D) for D in dc.DISTANCE_EDGES + dc.FAR_DISTANCE_EDGES} == set(range(30))
    assert C_ < 32768 or 24577 in edges
    for D in edges:
        text = dc.distance_edge(D)
        assert len(text) == (40 if D < 8 else D + 8)
        for rule in RULES:
            last = rule(text)[-1]
            assert not isinstance(last, int) and last[1] == D and (D < 8 or last[0] == 8), (D, rule.__name__, last)


def test_fibonacci_is_deeper_than_the_length_limit():
    ll, _ = dt.histograms(list(dc.fibonacci_counts(chunk_bytes())))
    assert ll[256] == 1 and dt.huffman(ll)[1] >= 17


def test_wide_tokens_reach_a_third_word():
    C_ = chunk_bytes()
    text = dc.wide_tokens(C_)
    assert len(text) <= C_
    assert dt.parse_host(text) == dt.parse_device(text)
    (m,) = dt.members(host_model(text, dc.DYNAMIC_ONLY))
    assert m.btype == dt.DYNAMIC and m.tokens == dt.parse_host(text)
    widths, third = dt.token_offsets(m)[1], dt.third_word_tokens(m)
    print(f"wide_tokens: {sum(w >= 34 for w in widths)} tokens of 34 bits or more, the widest {max(widths)}, "
          f"{len(third)} in three words")
    assert max(widths) >= 34 and len(third) >= 1


def test_every_length_symbol_in_one_chunk():
    text = dc.every_length_symbol()
    assert len(text) <= chunk_bytes()
    for rule in RULES:
        assert sorted(dt.length_symbol(t[0]) for t in _matches(rule(text))) == list(range(258, 286)), rule.__name__


# ---- the host model's members, token by token
@functools.lru_cache(maxsize=None)
def _audited(name):
    C_ = chunk_bytes()
    (case,) = [c for c in dc.cases(C_) if c[0] == name]
    return dc.audit(*case, host_model, dt.parse_host, C_)


def test_host_model_tokens_block_choice_and_codes(named):
    bad, _ = _audited(named[0])
    assert not bad, bad


def test_host_model_fibonacci_code_is_limited_to_15_bits():
    _, decoded = _audited("fibonacci")
    (m,) = decoded[dc.LITERALS_ONLY | dc.DYNAMIC_ONLY]
    ll, _ = dt.histograms(m.tokens)
    assert max(m.ll_len) == 15 and sum(f * n for f, n in zip(ll, m.ll_len)) >= dt.huffman(ll)[0]


def test_host_model_emits_every_symbol_from_its_named_case():
    C_ = chunk_bytes()
    names = [c[0] for c in dc.cases(C_) if c[0].startswith(("len", "dist")) or c[0] in ("wide_tokens", "every_length_symbol")]
    bad = dc.coverage_gaps({name: _audited(name)[1] for name in names}, C_)
    assert not bad, bad


def test_members_are_one_per_chunk_and_compress():
    C_ = chunk_bytes()
    data = dc.real_shapes(C_)["hashes_to_patterns"]
    members = host_model(data, 0)
    assert members.count(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff") >= -(-len(data) // C_)
    assert len(members) < len(data) // 3


def test_gzip_tool_accepts_a_multi_chunk_result(tmp_path):
    C_ = chunk_bytes()
    data = dc.real_shapes(C_)["kmers_to_hashes"]
    assert len(data) > 2 * C_
    p = tmp_path / "x.gz"
    p.write_bytes(host_model(data, 0))
    r = subprocess.run(["gzip", "-t", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gzip", "-dc", str(p)], capture_output=True)
    assert r.returncode == 0 and r.stdout == data


def test_writer_header_only_and_interleaved(tmp_path):
    p = tmp_path / "h.gz"
    with MemberGzipWriter(str(p)) as w:
        w.write("a\tb\n")
    with gzip.open(p, "rb") as fh:
        assert fh.read() == b"a\tb\n"
    rows1, rows2 = b"1\t2\n" * 5000, b"x\ty\n" * 70000
    q = tmp_path / "i.gz"
    w = MemberGzipWriter(str(q))
    write_text(w, "a\tb\n")
    m1, m2 = host_model(rows1, 0), host_model(rows2, 0)
    write_text(w, GzipMembers(memoryview(m1), len(rows1)))
    write_text(w, "host\trow\n")
    write_text(w, memoryview(b"bytes\trow\n"))
    write_text(w, GzipMembers(memoryview(m2)))              # (a stream's block: its text size is not known)
    write_text(w, GzipMembers(memoryview(b""), 0))
    w.close()
    with gzip.open(q, "rb") as fh:
        assert fh.read() == b"a\tb\n" + rows1 + b"host\trow\n" + b"bytes\trow\n" + rows2
    assert w.bytes_written == os.path.getsize(q) and 0 < w.header_bytes < 64
    # the members compressed here behind the header are counted apart from those handed in
    assert w.host_bytes > 0 and w.bytes_written == w.header_bytes + w.host_bytes + len(m1) + len(m2)


def test_cli_option_reaches_run(tmp_path):
    calls = []

    def stub(*a, **kw):
        calls.append((a, kw))
        return {"clusters": 0, "instances": 0, "patterns": 0, "log": ""}
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert cli.main(["-g", "gffs", "-p", "t.csv", "--gpu-compress"], run=stub) == 0
        assert cli.main(["-g", "gffs", "-p", "t.csv", "--compress"], run=stub) == 0
    finally:
        os.chdir(old)
    assert calls[0][1]["compress"] is True and calls[0][1]["device_gzip"] is True
    assert calls[1][1]["compress"] is True and "device_gzip" not in calls[1][1]
