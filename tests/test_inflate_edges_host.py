"""The device gunzip's format logic on the streams zlib never writes: its serial host model (pf_gunzip_host_model,
pf_gunzip_host_model_bgzf: the same inflate_blocks as the kernels, csrc/pf_deflate.h) over the hand-made members and the
seeded random members of tests/inflate_edges.py, what those inputs hold, and the two stand-alone sanitizer programs over
the whole set.  No GPU."""
import collections
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_tokens as dt  # noqa: E402
import inflate_edges as ie  # noqa: E402
import test_bgzf_host_model as tb  # noqa: E402
import test_inflate_host_model as ti  # noqa: E402

from panfeed_amd import _lib  # noqa: E402


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def host_gunzip(frame, data):
    """(text or None when not taken, the library's message) by the frame's host model"""
    return ti.host_gunzip(data) if frame == "plain" else tb.host_gunzip_bgzf(data)


@functools.lru_cache(maxsize=None)
def accepted():
    return ie.accepted(chunk_bytes())


@functools.lru_cache(maxsize=None)
def refused():
    return ie.refused(chunk_bytes())


@functools.lru_cache(maxsize=None)
def random_files():
    return ie.random_files(chunk_bytes())


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_accepted_cases_give_their_text(frame):
    items = [c for c in accepted() if c.frame == frame]
    assert len(items) >= 24
    bad = []
    for c in items:
        got, why = host_gunzip(frame, c.data)
        if got != c.text:
            bad.append(f"{c.name}: {why or ie.first_difference(got, c.text, c.marks)}")
    assert not bad, bad


def test_cases_hold_what_they_are_for():
    """beyond what every maker asserts of its own blocks: the frames, the sizes, the large frame's offsets"""
    C_ = chunk_bytes()
    items = accepted()
    names = {c.name for c in items if c.frame == "plain"}
    assert {c.name for c in items if c.frame == "bgzf"} == names and len(names) >= 25
    for k in range(8):
        assert f"stored_at_bit_offset_{k}" in names
    assert sum(n.startswith("overlap_grid") for n in names) >= 2
    for c in items:
        assert (len(c.text) > C_) == (c.frame == "bgzf64"), c.name
        assert len(c.data) <= (ie.ic.slot_bytes(C_) if c.frame == "plain" else ie.bc.MAX + 28), c.name
    assert sum(len(c.data) for c in items) + sum(len(r.data) for r in refused()) + sum(len(f[0]) for f in random_files().values()) < 2 << 20
    big = next(c for c in items if (c.name, c.frame) == ("every_symbol_extremes", "bgzf64"))
    assert any(isinstance(t, tuple) and t[:2] == (4, 32768) for _, _, t in big.marks)      # distance symbol 29 at its last value
    assert any(isinstance(t, tuple) and t[0] == 258 and len(t) == 3 and t[2] == 285 for _, _, t in big.marks)
    # the lone code, the missing code and the lone end-of-block code are in the streams as headers, not only as arguments
    for name in ("one_dist_code_1bit", "no_dist_code_literals", "only_eob_code_then_fixed"):
        c = next(c for c in items if (c.name, c.frame) == (name, "plain"))
        body = c.data[10:-8]
        hlit, hdist = (body[0] >> 3) + 257, (body[1] & 31) + 1
        assert body[0] & 6 == 4 and hdist == 1, name                   # BTYPE = 2, one distance length declared
        assert hlit == (257 if name != "one_dist_code_1bit" else 286)


def test_random_members_hold_what_they_are_for():
    """the seeded set's summary (ie.random_files asserts it as it makes the files): stated here once more on its own, and
    on a second draw the generator is the same"""
    members, summary = ie.random_members(ie.SEED, ie.N_RANDOM)
    ie.check_summary(summary)
    assert len(members) == 200 and all(1 <= len(t) <= 4096 for _, _, t, _ in members)
    again, _ = ie.random_members(ie.SEED, 5)
    assert [m[1] for m in again] == [m[1] for m in members[:5]]
    assert summary["lone_distance_blocks"] >= 5


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_random_members_give_their_text(frame):
    data, text, index = random_files()[frame]
    got, why = host_gunzip(frame, data)
    assert got == text, why or ie.where_in_file(got, text, index)


def test_refused_cases_name_the_member_and_the_check():
    items = refused()
    assert len({r.name for r in items if r.member == 0}) >= 23
    bad = []
    for r in items:
        got, why = host_gunzip(r.frame, r.data)
        if got is not None or not why.endswith(f"not taken: member {r.member}: {r.reason}"):
            bad.append(f"{r.name} ({r.frame}): {'taken' if got is not None else why}")
    assert not bad, bad


def test_refusals_cover_the_statuses():
    reasons = collections.Counter(r.reason for r in refused() if r.member == 0 and r.frame == "plain")
    assert reasons["bad symbol"] == 4 and reasons["ends before its tail"] == 1 and reasons["bad code lengths"] == 6
    assert reasons["bad code"] >= 7 and reasons["distance before the start"] == 2 and reasons["more text than ISIZE"] == 1
    # "bad code" against "truncated": a bit pattern no code has is named as such behind 15 or more bits of payload, and is
    # "truncated" within the payload's last 15 bits (InfStatus, csrc/pf_deflate.h)
    by = {r.name: r.reason for r in refused() if r.frame == "plain"}
    for name in ("one_dist_code_other_bit", "match_without_dist_code"):
        assert by[name] == "bad code" and by[name + "_at_the_end"] == "truncated"


def test_the_writer_agrees_with_the_token_reader():
    """the writer against tests/deflate_tokens.py's reader, which was written for the encoder's members: a one-block
    member's tokens, code lengths and text come back as they went in"""
    toks = list(b"abcab") + [(258, 3), 99, (3, 1), (17, 200)]
    for blk in (ie.fixed(toks, True), ie.dynamic(toks, ie.FULL_LL, ie.FULL_D, True)):
        w = ie.write([blk])
        m, = dt.members(ie.ic.wrap(w.body, w.text))
        assert m.tokens == toks and m.text == w.text and m.btype == blk["type"]
        if blk["type"] == dt.DYNAMIC:
            assert (m.ll_len, m.d_len) == (ie.FULL_LL, ie.FULL_D)
        assert [at for at, _, _ in w.marks] == [0, 1, 2, 3, 4, 5, 263, 264, 267]
    assert ie.token_at(w.marks, 262)[2] == (258, 3) and ie.token_at(w.marks, 263)[2] == 99


@pytest.mark.parametrize("frame", ["plain", "bgzf"])
def test_sanitizer_program_over_the_same_set(tmp_path, frame):
    """tools/inflate_host_check.cpp and tools/bgzf_host_check.cpp under AddressSanitizer and UBSan over the hand-made and
    the random members: every payload and every window is a heap buffer of its exact size there, so a 15-bit peek past a
    payload's last byte or a copy past ISIZE stops the program.  This is the run that comes before any of these inputs
    reaches a GPU."""
    import subprocess
    cc = ti._compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build the check programs with")
    tool = "inflate_host_check" if frame == "plain" else "bgzf_host_check"
    exe, cases = str(tmp_path / tool), str(tmp_path / "edge_cases.bin")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-DPF_GZ_CHUNK={chunk_bytes()}"]
    r = subprocess.run([cc] + flags + ["-I" + os.path.join(ti.REPO, "include"), os.path.join(ti.REPO, "tools", tool + ".cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cc} has no sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    files = random_files()
    extra = [(f"random-{f}", files[f][0], files[f][1]) for f in ie.FRAMES if (f == "plain") == (frame == "plain")]
    n_ok, n_bad = ie.dump(cases, accepted(), refused(), frame, extra)
    assert n_ok >= 26 and n_bad >= 46
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and int(r.stdout.split()[0]) >= n_ok + n_bad
