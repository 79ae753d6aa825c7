"""The device gunzip's format logic, run by its serial host model (pf_gunzip_host_model: the same host+device functions as
the kernel, csrc/pf_deflate.h) over the inputs of tests/inflate_cases.py, and the stand-alone sanitizer program over the
same set.  No GPU."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_cases as ic  # noqa: E402

from panfeed_amd import _lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def host_encode(data, flags):
    L = _lib.load()
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), flags, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def host_gunzip(members):
    """(text or None when not taken, the library's message)"""
    L = _lib.load()
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(L.pf_gunzip_host_model(members, len(members), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        if not taken.value:
            assert not out.value and n.value == 0
            return None, L.pf_last_error().decode()
        return (C.string_at(out, n.value) if n.value else b""), ""
    finally:
        L.pf_free_text(out)


@functools.lru_cache(maxsize=None)
def accepted():
    C_ = chunk_bytes()
    groups = {"encoder": ic.encoder_inputs(C_, host_encode), "layouts": ic.layout_inputs(C_, host_encode)}
    groups.update(ic.zlib_inputs(C_))
    return groups


GROUPS = ("encoder", "layouts", "zlib1", "zlib6", "zlib9", "zlib_sync")


@pytest.mark.parametrize("group", GROUPS)
def test_accepted_inputs_give_their_text(group):
    items = accepted()[group]
    assert len(items) >= 8
    bad = []
    for name, members, text in items:
        got, why = host_gunzip(members)
        if got != text:
            bad.append(f"{name}: {why or 'another text'}")
    assert not bad, bad


def test_inputs_hold_what_they_are_for():
    """the zlib inputs carry what this encoder never writes: run codes 16 / 17 / 18 (HLIT / HDIST below their largest
    values come with them), several blocks in a member, stored blocks in the middle of one"""
    import deflate_tokens as dt
    C_ = chunk_bytes()
    g = accepted()
    name, members, text = next(i for i in g["zlib9"] if i[0].endswith("shape_kmers_to_hashes"))
    ms = dt.members(members)
    assert len(ms) == -(-len(text) // C_) and all(m.btype == dt.DYNAMIC for m in ms[:-1])
    assert any(0 in m.ll_len[257:] or len(m.ll_len) < 286 for m in ms)
    # a sync flush ends a block, adds an empty stored one and goes on at a byte boundary: 00 00 FF FF twice a member
    name, members, text = next(i for i in g["zlib_sync"] if i[0].endswith("shape_kmers_to_hashes"))
    assert members.count(b"\x00\x00\xff\xff") >= 2 * -(-len(text) // C_)
    for _, members, _ in g["zlib1"] + g["zlib_sync"] + g["layouts"]:
        at = 0
        while at < len(members):                                     # every member fits the decoder's slot
            nxt = members.find(ic.HEAD, at + 1)
            nxt = len(members) if nxt < 0 else nxt
            assert nxt - at <= ic.slot_bytes(C_)
            at = nxt


def test_empty_input_is_taken():
    assert host_gunzip(b"") == (b"", "")


@functools.lru_cache(maxsize=None)
def refused():
    return ic.rejected(chunk_bytes(), host_encode)


def test_rejected_members_are_not_taken():
    items, ok = refused()
    assert host_gunzip(ok)[0] == b"a"
    assert len(items) >= 18
    bad = []
    for name, members in items:
        got, why = host_gunzip(members)
        if got is not None:
            bad.append(name)
        elif "not taken: member" not in why:
            bad.append(f"{name}: no reason given ({why!r})")
    assert not bad, bad


@pytest.mark.parametrize("name,member,reason", [
    ("match_before_start", 0, "distance before the start"), ("oversubscribed_literal_code", 0, "bad code"),
    ("incomplete_distance_code", 0, "bad code"), ("repeat_without_a_length", 0, "bad code lengths"),
    ("stored_len_nlen", 0, "stored LEN / NLEN"), ("no_end_of_block", 0, "truncated"), ("more_than_isize", 0, "more text than ISIZE"),
    ("block_type_3", 0, "block type 3"), ("wrong_crc", 0, "CRC32 differs"), ("isize_one_less", 0, "more text than ISIZE"),
    ("isize_one_more", 0, "less text than ISIZE"), ("isize_chunk_plus_1", 0, "too large"), ("payload_cut_tail_kept", 0, "truncated"),
    ("signature_in_stored_text", 0, "truncated"), ("bad_member_between_good_ones", 1, "CRC32 differs")])
def test_refusal_names_the_member_and_the_check(name, member, reason):
    """the hand-made members fail the check they were made for, not an earlier one"""
    members = dict(refused()[0])[name]
    got, why = host_gunzip(members)
    assert got is None and why.endswith(f"member {member}: {reason}"), why


def test_a_foreign_header_is_not_taken():
    import gzip
    assert host_gunzip(gzip.compress(b"text\n" * 10, mtime=5))[0] == b"text\n" * 10   # MTIME set: another signature is fine,
    whole = gzip.compress(b"x" * (chunk_bytes() + 1), mtime=0)                        # but a member over CHUNK is not
    assert host_gunzip(whole)[0] is None
    named = bytearray(gzip.compress(b"text\n", mtime=0))
    named[3] = 8                                                                      # FLG.FNAME
    assert host_gunzip(bytes(named))[0] is None


def _compiler():
    for cc in ("g++", "clang++"):
        if shutil.which(cc):
            return cc
    return None


def test_sanitizer_program_over_the_same_set(tmp_path):
    """tools/inflate_host_check.cpp under AddressSanitizer and UBSan: every payload and every window is a heap buffer of
    its exact size there, so a read past a member's last byte or a write past its ISIZE stops the program"""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build tools/inflate_host_check.cpp with")
    exe, cases = str(tmp_path / "inflate_host_check"), str(tmp_path / "inflate_cases.bin")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-DPF_GZ_CHUNK={chunk_bytes()}"]
    r = subprocess.run([cc] + flags + ["-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "inflate_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cc} has no sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    n_ok, n_bad = ic.dump(cases, chunk_bytes(), host_encode, [i for g in accepted().values() for i in g])
    assert n_ok > 100 and n_bad >= 18
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and int(r.stdout.split()[0]) >= n_ok + n_bad
