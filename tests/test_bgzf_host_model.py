"""BGZF without a GPU: the device decoder's host model for it (pf_gunzip_host_model_bgzf: list_members_bgzf and the same
inflate_blocks as the kernels, csrc/pf_deflate.h) over the files of tests/bgzf_cases.py, the encoder's framing under
PF_GZ_BGZF by its host model, the stand-alone sanitizer program over the same files, output.BgzfMemberWriter and the
refusals of `panfeed --bgzf`."""
import ctypes as C
import functools
import gzip
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgzf_cases as bc  # noqa: E402

from panfeed_amd import _lib, cli  # noqa: E402
from panfeed_amd.output import BgzfMemberWriter  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def _taken(call, data):
    """(text or None when not taken, the library's message) of a pf_gunzip_* call"""
    L = _lib.load()
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(call(data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        if not taken.value:
            assert not out.value and n.value == 0
            return None, L.pf_last_error().decode()
        return (C.string_at(out, n.value) if n.value else b""), ""
    finally:
        L.pf_free_text(out)


def host_gunzip_bgzf(data):
    return _taken(_lib.load().pf_gunzip_host_model_bgzf, data)


def host_encode(data, flags):
    L = _lib.load()
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(L.pf_gzip_host_model(data, len(data), flags, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


@functools.lru_cache(maxsize=None)
def accepted():
    return bc.accepted(chunk_bytes())


@functools.lru_cache(maxsize=None)
def refused():
    return bc.refused(chunk_bytes())


def test_accepted_files_give_their_text():
    items = accepted()
    assert len(items) >= 20
    bad = [f"{name}: {why or 'another text'}" for name, data, text in items for got, why in [host_gunzip_bgzf(data)] if got != text]
    assert not bad, bad


def test_files_hold_what_they_are_for():
    """members of more text than the plain decoder's chunk, stored members of bgzip's block size, several blocks in one"""
    items = {name: (data, text) for name, data, text in accepted()}
    sizes = [len(t) for _, _, t in bc.walk(items["tsv_300k_level6"][0])]
    assert sizes[:4] == [bc.BLOCK] * 4 and sizes[-1] == 0 and bc.BLOCK > chunk_bytes()
    stored = bc.walk(items["stored_65280_blocks"][0])
    assert all(size > bc.BLOCK for _, size, t in stored[:-1])
    assert items["sync_flush_inside"][0].count(b"\x00\x00\xff\xff") >= 4
    assert len(bc.walk(items["one_member_65536"][0])) == 2 and len(items["one_member_65536"][1]) == bc.MAX


def test_refused_files_name_the_member_and_the_check():
    items = refused()
    assert len(items) >= 11
    bad = []
    for name, data, member, reason in items:
        got, why = host_gunzip_bgzf(data)
        if got is not None or not why.endswith(f"not taken: member {member}: {reason}"):
            bad.append(f"{name}: {'taken' if got is not None else why}")
    assert not bad, bad


def test_the_plain_entry_point_still_refuses_bgzf():
    """pf_gunzip_host_model keeps its header: FLG = 0 only"""
    data = next(d for n, d, _ in accepted() if n == "one_member_1")
    got, why = _taken(_lib.load().pf_gunzip_host_model, data)
    assert got is None and why.endswith("member 0: bad header")
    got, why = host_gunzip_bgzf(gzip.compress(b"text\n", mtime=0))
    assert got is None and why.endswith("member 0: bad header")


@pytest.mark.parametrize("n", ["0", "1", "C-1", "C+1", "3C+17"])
def test_encoder_framing_by_the_host_model(n):
    """under PF_GZ_BGZF every member is the unflagged member with its bytes from 10 on behind the 18-byte head"""
    C_ = chunk_bytes()
    text = bc.tsv_text({"0": 0, "1": 1, "C-1": C_ - 1, "C+1": C_ + 1, "3C+17": 3 * C_ + 17}[n], seed=9)
    plain, framed = host_encode(text, 0), host_encode(text, _lib.GZ_BGZF)
    assert gzip.decompress(framed + bc.EOF) == text
    members = bc.walk(framed + bc.EOF)
    assert b"".join(t for _, _, t in members) == text and len(members) == -(-len(text) // C_) + 1
    at = 0
    for off, size, _ in members[:-1]:
        one = plain[at:at + size - 8]
        head = one[:3] + b"\x04" + one[4:10] + struct.pack("<H2sHH", 6, b"BC", 2, size - 1)
        assert framed[off:off + size] == head + one[10:]
        at += size - 8
    assert at == len(plain)
    assert host_gunzip_bgzf(framed + bc.EOF) == (text, "") and host_gunzip_bgzf(framed) == (text, "")


def _compiler():
    for cc in ("g++", "clang++"):
        if shutil.which(cc):
            return cc
    return None


def test_sanitizer_program_over_the_same_files(tmp_path):
    """tools/bgzf_host_check.cpp under AddressSanitizer and UBSan: every payload and every window of up to 64 KiB is a
    heap buffer of its exact size there"""
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++ / clang++) to build tools/bgzf_host_check.cpp with")
    exe, cases = str(tmp_path / "bgzf_host_check"), str(tmp_path / "bgzf_cases.bin")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-DPF_GZ_CHUNK={chunk_bytes()}"]
    r = subprocess.run([cc] + flags + ["-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "bgzf_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and ("cannot find" in r.stderr or "unsupported" in r.stderr):
        pytest.skip(f"{cc} has no sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    n_ok, n_bad = bc.dump(cases, accepted(), refused())
    assert n_ok >= 20 and n_bad >= 11
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and int(r.stdout.split()[0]) >= n_ok + n_bad


# ---- the writer
def _written(tmp_path, fill):
    path = str(tmp_path / "t.tsv.gz")
    w = BgzfMemberWriter(path)
    fill(w)
    w.close()
    with open(path, "rb") as fh:
        data = fh.read()
    assert w.bytes_written == len(data)
    return data, w


def test_writer_header_only(tmp_path):
    data, w = _written(tmp_path, lambda w: w.write("cluster\tstrain\n"))
    assert [t for _, _, t in bc.walk(data)] == [b"cluster\tstrain\n", b""]
    assert w.header_bytes == len(data) - 28 and w.host_bytes == 0
    assert bc.walk(_written(tmp_path, lambda w: None)[0]) == [(0, 28, b"")]


def test_writer_cuts_host_text_into_bgzf_blocks(tmp_path):
    text = bc.tsv_text(200000, seed=3)
    data, w = _written(tmp_path, lambda w: (w.write("head\n"), w.write(text)))
    members = bc.walk(data)
    assert [len(t) for _, _, t in members] == [5, 65280, 65280, 65280, 200000 - 3 * 65280, 0]
    assert gzip.decompress(data) == b"head\n" + text
    assert w.host_bytes == len(data) - w.header_bytes - 28
    assert host_gunzip_bgzf(data) == (b"head\n" + text, "")


def test_writer_interleaves_device_members(tmp_path):
    C_ = chunk_bytes()
    a, b, c = bc.tsv_text(C_ + 5, seed=4), bc.tsv_text(70000, seed=5), bc.tsv_text(3, seed=6)

    def fill(w):
        w.write("head\n")
        w.write_members(memoryview(host_encode(a, _lib.GZ_BGZF)))
        w.write(b)
        w.write_members(host_encode(c, _lib.GZ_BGZF))
        w.write_members(b"")
    data, w = _written(tmp_path, fill)
    assert [len(t) for _, _, t in bc.walk(data)] == [5, C_, 5, 65280, 70000 - 65280, 3, 0]
    assert gzip.decompress(data) == b"head\n" + a + b + c
    assert host_gunzip_bgzf(data) == (b"head\n" + a + b + c, "")


# ---- the command line
@pytest.mark.parametrize("extra,env", [
    ([], {}),                                                        # without --gpu-compress
    (["--compress"], {}),
    (["--gpu-compress", "--multiple-files"], {}),
    (["--gpu-compress", "--gpus", "2"], {}),
    (["--gpu-compress"], {"WORLD_SIZE": "2", "RANK": "0"}),         # as a launched rank
])
def test_bgzf_refusals_read_no_file(tmp_path, monkeypatch, extra, env):
    calls = []
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.chdir(tmp_path)
    stand_in = lambda *a, **kw: calls.append((a, kw)) or {}          # noqa: E731
    rc = cli.main(["-g", "gffs", "-p", "table.csv", "--targets", "no_such_file.txt", "--bgzf"] + extra, run=stand_in,
                  launch=stand_in, rank_entry=stand_in)
    assert rc == 2 and not calls and os.listdir(tmp_path) == []


def test_bgzf_reaches_run_files(tmp_path, monkeypatch):
    calls = []
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["-g", "gffs", "-p", "table.csv", "--gpu-compress", "--bgzf"], run=lambda *a, **kw: calls.append(kw) or {})
    assert rc == 0 and calls[0]["device_gzip"] is True and calls[0]["bgzf"] is True and calls[0]["compress"] is True
