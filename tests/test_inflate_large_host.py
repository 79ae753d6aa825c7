"""The large-member gunzip route without a GPU: its serial host model (pf_gunzip_host_model_large: the find, marker, chain
and byte steps from the functions the kernels run, csrc/pf_deflate.h) over the files of tests/inflate_large_cases.py, what
those files hold, the switch's plumbing in Python, and the stand-alone sanitizer program over the same set."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_large_cases as lc  # noqa: E402
import test_inflate_host_model as ti  # noqa: E402

from panfeed_amd import _lib, downstream  # noqa: E402


def host_large(data, piece_bytes):
    """(text or None when not taken, [found, live, dropped, members], the library's message)"""
    L = _lib.load()
    out, n, taken, pieces = C.c_void_p(), C.c_uint64(), C.c_int(), (C.c_uint64 * 4)()
    _lib.check(L.pf_gunzip_host_model_large(data, len(data), piece_bytes, C.byref(out), C.byref(n), C.byref(taken), pieces))
    try:
        if not taken.value:
            assert not out.value and n.value == 0
            return None, list(pieces), L.pf_last_error().decode()
        return (C.string_at(out, n.value) if n.value else b""), list(pieces), ""
    finally:
        L.pf_free_text(out)


@functools.lru_cache(maxsize=None)
def accepted():
    return lc.accepted(ti.host_encode)


@functools.lru_cache(maxsize=None)
def refused():
    return lc.refused()


@functools.lru_cache(maxsize=None)
def host_results():
    """every (case, piece_bytes) through the host model, once: the GPU tests compare the device's counts with these"""
    return {(c.name, p): host_large(c.data, p) for c in accepted() for p in c.pieces}


def test_accepted_files_give_zlib_s_text():
    assert len(accepted()) >= 15
    bad = [f"{name} at {p}: {why or 'another text'}" for (name, p), (got, _, why) in host_results().items()
           if got != next(c for c in accepted() if c.name == name).text]
    assert not bad, bad


def test_files_hold_what_they_are_for():
    r = host_results()
    for name in ("zlib1_mem1", "zlib6_mem1", "zlib9_mem1", "sync_flush"):
        found, live, dropped, members = r[name, 64][1]
        assert found >= 20 and live == found and dropped == 0 and members == 1, name      # tens of pieces, no false start
    for name in ("fixed_only", "stored_only"):
        assert r[name, 64][1] == [1, 1, 0, 1], name                                          # nothing found: one piece
    assert b"\x00\x00\xff\xff" in next(c for c in accepted() if c.name == "sync_flush").data
    found, live, dropped, members = r["handmade_chain", 64][1]
    assert (found, live, dropped) == (5, 5, 0)                                                # each block a piece
    for p in lc.PIECES:
        found, live, dropped, members = r["stored_stream_inside", p][1]
        assert dropped > 0 and live + dropped == found and live <= 3, p                       # the false starts are dropped
    assert r["two_members_two_heads", 64][1][3] == 2 and r["large_between_small", 64][1][3] >= 3
    for p in (64, 512):                                                                       # every member taken, in several calls
        assert r["many_tiny_members", p][1] == [lc.MANY, lc.MANY, 0, lc.MANY], p
    assert r["large_members_in_a_row", 64][1][3] == 4 and r["large_members_in_a_row", 64][1][2] == 0
    assert all(r[name, 0][1][:3] == [1, 1, 0] for name in lc.DEFAULT_TOO)                     # under 32 KiB compressed: one piece
    w = lc.handmade_blocks()
    toks = [t for _, _, t in w.marks if isinstance(t, tuple)]
    assert toks.count((258, lc.WINDOW)) == 2 and (200, 3) in toks and toks[-1] == (258, 5)


def test_refused_files_are_not_taken_and_say_why():
    assert len(refused()) >= 7
    bad = []
    for r in refused():
        for p in r.pieces:
            got, _, why = host_large(r.data, p)
            if got is not None or "not taken: member 0: " not in why:
                bad.append(f"{r.name} at {p}: {'taken' if got is not None else why}")
    assert not bad, bad
    why = {r.name: host_large(r.data, 64)[2].rsplit(": ", 1)[1] for r in refused()}
    assert why["reserved_flg_bit"] == why["cm_not_8"] == "bad header"
    assert why["cut_in_last_block"] == why["cut_in_tail"] == "truncated"
    assert why["match_before_start"] == "distance before the start"
    assert (why["isize_one_more"], why["isize_one_less"]) == ("less text than ISIZE", "more text than ISIZE")


def test_piece_bytes_is_zero_or_at_least_64():
    L = _lib.load()
    data = accepted()[0].data
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    assert L.pf_gunzip_host_model_large(data, len(data), 63, C.byref(out), C.byref(n), C.byref(taken), None) == _lib.ERR_ARG
    assert host_large(data, 64)[0] == host_large(data, 0)[0] == accepted()[0].text
    assert host_large(b"", 64)[0] == b""


def test_the_automatic_route_tries_other_heads_only_with_the_switch(tmp_path):
    """route_file's choice, with stand-ins for the two ways: a gzip.open file (FLG = FNAME) goes to members() only under
    large_members; --host-gunzip's device_gunzip=False never does"""
    path = tmp_path / "named.tsv.gz"
    with gzip.open(path, "wb") as fh:
        fh.write(b"a\tb\n")
    assert path.read_bytes()[3] == lc.FNAME

    class Counts:
        device_gunzip_files = fallback_files = 0

    calls = []
    go = lambda **kw: downstream.route_file(str(path), kw.pop("device_gunzip", None), lambda: calls.append("members") or "m",     # noqa: E731
                                            lambda: calls.append("host") or "h", Counts, **kw)
    assert go() == "h" and go(large_members=False) == "h" and calls == ["host", "host"]
    assert go(large_members=True) == "m" and calls[-1] == "members" and Counts.device_gunzip_files == 1
    assert go(large_members=True, device_gunzip=False) == "h" and calls[-1] == "host"
    plain = tmp_path / "plain.tsv"
    plain.write_bytes(b"a\tb\n")
    assert not downstream._gz_any_file(str(plain)) and downstream._gz_any_file(str(path))


def test_the_tools_have_the_flag(capsys):
    from panfeed_amd import plot
    for kmers in (False, True):
        p = downstream._options("x", kmers)
        assert any("--gpu-gunzip-large" in a.option_strings for a in p._actions)
        assert "--host-gunzip wins" in p.format_help()
    with pytest.raises(SystemExit):
        plot.get_options(["--help"])
    assert "--gpu-gunzip-large" in capsys.readouterr().out


def test_sanitizer_program_over_the_same_set(tmp_path):
    """tools/inflate_large_host_check.cpp under AddressSanitizer and UBSan: every pass reads a heap copy of exactly the
    call's bytes, every ring and every piece's text is a heap buffer of its exact size; the cases go through whole and in
    blocks of 4 096 bytes, and the finder and the marker sink start at every bit offset of the random streams and of three
    distinct real ones, whole and cut short (the program names them)"""
    cc = ti._compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build the check program with")
    exe, cases = str(tmp_path / "inflate_large_host_check"), str(tmp_path / "large_cases.bin")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cc] + flags + ["-I" + os.path.join(ti.REPO, "include"), os.path.join(ti.REPO, "tools", "inflate_large_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cc} has no sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    n_ok, n_bad = lc.dump(cases, accepted(), refused())
    assert n_ok >= 48 and n_bad >= 21
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and int(r.stdout.splitlines()[-1].split()[0]) >= 2 * (n_ok + n_bad)
    assert "every bit offset of: fixed_only handmade_chain head_fextra" in r.stdout
