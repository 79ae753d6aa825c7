"""The device gunzip (pf_gunzip_device: one wave per gzip member, csrc/pf_deflate.hip) over the inputs of
tests/inflate_cases.py: members from the device encoder, from the encoder's host model and from zlib, member layouts,
and members that must be refused."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import inflate_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def _text(L, call):
    from panfeed_amd import _lib
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(call(C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def device_gzip(eng, data, flags):
    return _text(eng.L, lambda out, n: eng.L.pf_gzip_device(eng.ctx, data, len(data), flags, out, n))


def host_gzip(eng, data, flags):
    return _text(eng.L, lambda out, n: eng.L.pf_gzip_host_model(data, len(data), flags, out, n))


def _gunzip(L, call):
    """(text or None when not taken, the library's message)"""
    taken = C.c_int()
    text = _text(L, lambda out, n: call(out, n, C.byref(taken)))
    return (text, "") if taken.value else (None, L.pf_last_error().decode())


def device_gunzip(eng, members):
    return _gunzip(eng.L, lambda out, n, taken: eng.L.pf_gunzip_device(eng.ctx, members, len(members), out, n, taken))


def host_gunzip(eng, members):
    return _gunzip(eng.L, lambda out, n, taken: eng.L.pf_gunzip_host_model(members, len(members), out, n, taken))


def _all_give_their_text(eng, items):
    bad = []
    for name, members, text in items:
        got, why = device_gunzip(eng, members)
        if got != text:
            bad.append(f"{name}: {why or 'another text'}")
    assert not bad, bad


def test_members_of_the_device_encoder(eng):
    items = ic.encoder_inputs(chunk_bytes(), lambda data, flags: device_gzip(eng, data, flags))
    assert len(items) > 100
    _all_give_their_text(eng, items)


def test_members_of_the_host_model(eng):
    _all_give_their_text(eng, ic.encoder_inputs(chunk_bytes(), lambda data, flags: host_gzip(eng, data, flags)))


@pytest.fixture(scope="module")
def zlib_inputs():
    return ic.zlib_inputs(chunk_bytes())


@pytest.mark.parametrize("group", ["zlib1", "zlib6", "zlib9", "zlib_sync"])
def test_members_of_zlib(eng, zlib_inputs, group):
    assert len(zlib_inputs[group]) > 50
    _all_give_their_text(eng, zlib_inputs[group])


def test_member_layouts(eng):
    _all_give_their_text(eng, ic.layout_inputs(chunk_bytes(), lambda data, flags: device_gzip(eng, data, flags)))
    assert device_gunzip(eng, b"") == (b"", "")


@pytest.mark.parametrize("shape", ["kmers_to_hashes", "hashes_to_patterns", "kmers_tsv"])
def test_round_trip_of_the_files_rows(eng, shape):
    text = dc.real_shapes(chunk_bytes())[shape]
    members = device_gzip(eng, text, 0)
    assert device_gunzip(eng, members) == (text, "")
    ms = C.c_float(-1)
    assert eng.L.pf_gunzip_device_last_ms(eng.ctx, C.byref(ms)) == 0 and ms.value > 0


def test_rejected_members_are_not_taken_and_leave_nothing_behind(eng):
    """every refused input comes back not taken, with the host model's reason, and a good input decoded right behind it
    in the same context still gives its text.  An input goes to the device only after the host model (the same
    functions, which tests/test_inflate_host_model.py also runs under a sanitizer) has refused it."""
    C_ = chunk_bytes()
    items, ok = ic.rejected(C_, lambda data, flags: host_gzip(eng, data, flags))
    good_text = dc.real_shapes(C_)["kmers_tsv"][:C_ + 99]
    good = device_gzip(eng, good_text, 0)
    bad = []
    for name, members in items:
        on_host, why_host = host_gunzip(eng, members)
        assert on_host is None, name
        got, why = device_gunzip(eng, members)
        if got is not None:
            bad.append(f"{name}: taken")
        elif why.split("not taken: ")[-1] != why_host.split("not taken: ")[-1]:
            bad.append(f"{name}: {why!r} on the device, {why_host!r} by the host model")
        if device_gunzip(eng, good) != (good_text, ""):
            bad.append(f"{name}: the good input behind it")
    assert not bad, bad
    assert device_gunzip(eng, ok) == (b"a", "")
