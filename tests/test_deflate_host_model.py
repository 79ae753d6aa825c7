"""The gzip container and deflate coder of the device encoder, run by its serial host model (pf_gzip_host_model: the same
host+device format functions as the kernel, csrc/pf_deflate.h) on the cases of tests/deflate_cases.py; the .gz writer that
takes host text and ready members; the --gpu-compress option.  No GPU."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402

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


def test_host_model_decodes_to_the_input(case):
    name, data, flags = case
    C_ = chunk_bytes()
    members = host_model(data, flags)
    dc.check_members(data, members, C_)
    if name.startswith("incompressible"):
        assert len(members) <= dc.incompressible_cap(len(data), C_)


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
