"""The device gzip encoder's second effort level (PF_GZ_DEEP) run by the serial host model (pf_gzip_host_model: the rule
is written once, csrc/pf_deflate.h, for the model and the kernel) on the edge texts of tests/deflate_deep_model.py and on
every case of tests/deflate_cases.py: the members decode to the text, their tokens are the rule's (parse_host_deep), the
block type is the smallest, the codes are complete; level 2 is no larger than level 1 on the three real shapes and no
larger than zlib's level ZLIB_LEVEL on hashes_to_patterns, plain and as BGZF.  No GPU."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_deep_model as dd  # noqa: E402
import deflate_tokens as dt  # noqa: E402

from panfeed_amd import _lib  # noqa: E402


def host_model(data, flags):
    L = _lib.load()
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), flags, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def host_model_segments(data, ends, flags):
    L = _lib.load()
    out, n = C.c_void_p(), C.c_uint64()
    seg = (C.c_uint64 * len(ends))(*ends)
    member_end = (C.c_uint64 * len(ends))()
    _lib.check(L.pf_gzip_host_model_segments(data, len(data), seg, len(ends), flags, C.byref(out), C.byref(n), member_end))
    try:
        return (C.string_at(out, n.value) if n.value else b""), list(member_end)
    finally:
        L.pf_free_text(out)


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def test_the_flag():
    assert _lib.GZ_DEEP == dd.DEEP == 16 and _lib.GZ_BGZF == dd.BGZF
    assert _lib.gzip_level_flags(1) == 0 and _lib.gzip_level_flags(2) == _lib.GZ_DEEP
    for bad in (0, 3, None, True, "2"):
        with pytest.raises(ValueError):
            _lib.gzip_level_flags(bad)


def pytest_generate_tests(metafunc):
    if "named" in metafunc.fixturenames:
        C_ = chunk_bytes()
        named = list(dd.deep_cases(C_)) + [(f"cases_{name}", data) for name, data, _ in dc.cases(C_)]
        metafunc.parametrize("named", named, ids=[c[0] for c in named])


def test_tokens_block_choice_and_codes(named):
    """under DEEP, DEEP | FIXED_ONLY and DEEP | DYNAMIC_ONLY: Python's gzip gives back the text, and the audit finds the
    rule's tokens, the smallest block type and complete codes"""
    name, data = named
    C_ = chunk_bytes()
    for flags in dd.DEEP_FLAGS:
        members = host_model(data, flags)
        dc.check_members(data, members, C_)
        if name == "cases_incompressible" and flags == dd.DEEP:
            assert len(members) <= dc.incompressible_cap(len(data), C_)
    bad, _ = dd.audit_deep(name.replace("cases_", ""), data, lambda d, f: host_model(d, f | dd.DEEP), dd.parse_host_deep, C_)
    assert not bad, (len(bad), bad[:10])


def test_literals_only_wins():
    C_ = chunk_bytes()
    for name, data in dd.deep_cases(C_):
        if name.startswith("shape_"):
            data = data[:C_ + 77]
        for more in (0, dc.DYNAMIC_ONLY):
            assert host_model(data, dd.DEEP | dc.LITERALS_ONLY | more) == host_model(data, dc.LITERALS_ONLY | more), name


def test_default_is_not_the_deep_rule():
    """flags == 0 keeps the level-1 tokens on a text where the two rules differ"""
    C_ = chunk_bytes()
    text = dc.real_shapes(C_)["hashes_to_patterns"][:C_]
    (one,), (two,) = dt.members(host_model(text, 0)), dt.members(host_model(text, dd.DEEP))
    assert one.tokens == dt.parse_host(text) and two.tokens == dd.parse_host_deep(text) and one.tokens != two.tokens


def _tokens(name, flags=dd.DEEP):
    C_ = chunk_bytes()
    data = dict(dd.deep_cases(C_))[name]
    return data, [m.tokens for m in dt.members(host_model(data, flags))]


def test_three_byte_match_near_and_far():
    """length symbol 257 is emitted for the 3-byte agreement 4 096 bytes back and not for the one 4 097 back"""
    _, (near,) = _tokens("three_bytes_near")
    _, (far,) = _tokens("three_bytes_far")
    assert (3, 4096) in near
    assert not any(not isinstance(t, int) and t[0] == 3 for t in far)


def test_match_longer_than_max_match_at_distance_301():
    _, (tokens,) = _tokens("equal_rows_300")
    at = tokens.index((258, 301))
    assert tokens[at + 1][1] == 301                           # (the match goes on behind MAX_MATCH)


def test_row_candidate_is_not_taken_behind_the_previous_rows_end():
    """the host model's tokens on unequal_rows are the rule's, and the rule's are not those of a B taken on or behind the
    previous row's '\\n' (the text is built so that such a B would match to the row's end)"""
    data, (tokens,) = _tokens("unequal_rows")
    assert tokens == dd.parse_host_deep(data)
    assert tokens != dd._deep(data, dd._cands_host(data), False, "noclause")
    s, r = dd.row_starts(data)[22 + 25]       # column 25 of the second row: the first row has 21 columns
    assert (s, r) == (22, 0) and dd.row_candidate(22 + 25, s, r) is None and dd.row_candidate(22 + 5, s, r) == 5
    assert dd.row_candidate(22 + 20, s, r) == 20 and dd.row_candidate(22 + 21, s, r) is None      # (on the '\\n' itself)


ROW_CASES = ("long_rows", "equal_rows_300", "unequal_rows", "lazy_through_b_at_255", "lazy_through_b_at_511") + tuple(
    f"newline_at_{at}" for at in (63, 64, 191, 192, 255, 256, 257))


@pytest.mark.parametrize("name", ROW_CASES)
def test_row_cases_catch_what_they_are_for(name):
    """each text of rows is one on which only candidate B finds the long matches: the host model's tokens are the rule's,
    and the rule's differ from level 1's, from those without B, with B off by one either way and with any one of the
    newlines that have text behind them overlooked"""
    data, (tokens,) = _tokens(name)
    assert tokens == dd.parse_host_deep(data) and tokens != dt.parse_host(data)
    newlines = [i for i in dd._newlines(data) if i + 1 < len(data)]
    if name.startswith("lazy_through_b_at_"):
        newlines = [i for i in newlines if i <= int(name.rsplit("_", 1)[1])]
    if name == "equal_rows_300":              # (equal rows: without the second '\n' the third row's B is the same byte)
        newlines = newlines[:1]
    assert dd.differs_from_mutants(data, dd.B_MUTANTS + tuple(("drop", i) for i in newlines))


@pytest.mark.parametrize("name,at", [("lazy_at_255", (255,)), ("lazy_at_511", (511,)), ("lazy_chain", (300, 301, 302)),
                                     ("lazy_through_b_at_255", (255,)), ("lazy_through_b_at_511", (511,))])
def test_deferrals_where_the_cases_put_them(name, at):
    data, (tokens,) = _tokens(name)
    assert tokens == dd.parse_host_deep(data)
    got = dd.deferrals(data, dd.parse_host_deep)
    assert all(q in got for q in at), got


def test_deferral_before_the_texts_last_match():
    data, (tokens,) = _tokens("lazy_at_n_minus_2")
    assert len(data) - 5 in dd.deferrals(data, dd.parse_host_deep) and tokens[-1][0] == 4 and tokens[-2] == data[-5]


def test_chunk_that_starts_inside_a_row():
    """two segments, the first of an odd length that ends inside a row: every segment's members are those of its text
    alone, and the second segment's tokens are the rule's on its own bytes -- a misaligned candidate B, nothing worse"""
    C_ = chunk_bytes()
    text, ends = dd.segment_case(C_)
    members, member_end = host_model_segments(text, ends, dd.DEEP)
    assert member_end[-1] == len(members)
    at = 0
    for lo, hi, end in zip([0] + ends[:-1], ends, member_end):
        assert members[at:end] == host_model(text[lo:hi], dd.DEEP)
        assert [m.tokens for m in dt.members(members[at:end])] == [dd.parse_host_deep(c) for c in dc.chunks_of(text[lo:hi], C_)]
        at = end


def _sizes(encode, frame):
    C_ = chunk_bytes()
    out = {}
    for shape, text in dc.real_shapes(C_).items():
        one, two = len(encode(text, 0)), len(encode(text, dd.DEEP))
        z = {level: dd.zlib_total(text, C_, level, frame) for level in (1, 4, 6, 9)}
        print(f"{shape}: {len(text)} bytes of text, level 1 {one}, level 2 {two}, zlib 1/4/6/9 on the same cuts {z}")
        out[shape] = (one, two, z)
    return out


@pytest.mark.parametrize("bgzf", [0, dd.BGZF], ids=["plain", "bgzf"])
def test_level_2_sizes(bgzf):
    """on each of the three real shapes level 2 is no larger than level 1; on hashes_to_patterns it is no larger than
    zlib's level ZLIB_LEVEL on the same cuts (under BGZF both count the frames, 8 bytes a member)"""
    sizes = _sizes(lambda d, f: host_model(d, f | bgzf), 8 if bgzf else 0)
    for shape, (one, two, z) in sizes.items():
        assert two <= one, shape
    one, two, z = sizes["hashes_to_patterns"]
    assert two <= z[dd.ZLIB_LEVEL]


def test_zlib_level_is_the_highest_beaten_by_two_percent():
    """how ZLIB_LEVEL was chosen, kept checkable: the highest of 1, 4, 6, 9 whose total the host model's level 2 is at
    least 2 % under on hashes_to_patterns"""
    C_ = chunk_bytes()
    text = dc.real_shapes(C_)["hashes_to_patterns"]
    two = len(host_model(text, dd.DEEP))
    beaten = [level for level in (1, 4, 6, 9) if two <= 0.98 * dd.zlib_total(text, C_, level)]
    assert beaten and max(beaten) == dd.ZLIB_LEVEL, (two, beaten)
