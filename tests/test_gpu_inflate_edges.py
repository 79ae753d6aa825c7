"""The device gunzip (gz_inflate_kernel, gz_inflate64_kernel; csrc/pf_deflate.hip) on the streams zlib never writes: the
hand-made members and the seeded random members of tests/inflate_edges.py, through pf_gunzip_device (the plain container)
and pf_gunzip_device_bgzf (BGZF members of at most a chunk of text, and of more).  The expected text is the writer's own
byte-serial expansion, which zlib has confirmed.  Nothing goes to the device that the host model -- the same functions,
which tests/test_inflate_edges_host.py also runs under a sanitizer -- has not passed over first."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_edges as ie  # noqa: E402

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


def _gunzip(L, call):
    """(text or None when not taken, the library's message)"""
    from panfeed_amd import _lib
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(call(C.byref(out), C.byref(n), C.byref(taken)))
    try:
        text = C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)
    return (text, "") if taken.value else (None, L.pf_last_error().decode())


def device_gunzip(eng, frame, data):
    call = eng.L.pf_gunzip_device if frame == "plain" else eng.L.pf_gunzip_device_bgzf
    return _gunzip(eng.L, lambda out, n, taken: call(eng.ctx, data, len(data), out, n, taken))


def host_gunzip(eng, frame, data):
    call = eng.L.pf_gunzip_host_model if frame == "plain" else eng.L.pf_gunzip_host_model_bgzf
    return _gunzip(eng.L, lambda out, n, taken: call(data, len(data), out, n, taken))


@pytest.fixture(scope="module")
def accepted():
    return ie.accepted(chunk_bytes())


@pytest.fixture(scope="module")
def random_files():
    return ie.random_files(chunk_bytes())


def _differences(eng, cases):
    """every case whose device text is not the writer's: the first differing offset and the token that wrote it -- for a
    match, its (len, dist)"""
    bad = []
    for c in cases:
        assert host_gunzip(eng, c.frame, c.data) == (c.text, ""), c.name
        got, why = device_gunzip(eng, c.frame, c.data)
        if got != c.text:
            bad.append(f"{c.name}: {why or ie.first_difference(got, c.text, c.marks)}")
    return bad


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_accepted_cases_give_their_text(eng, accepted, frame):
    """the lone distance code, the block without one, codes of 15 bits mid-stream and as the payload's last bits, 258 as
    symbol 284, the run codes, tables that follow one another, stored blocks at the eight bit offsets"""
    cases = [c for c in accepted if c.frame == frame and not c.name.startswith(("overlap_grid", "every_symbol", "hlit_286"))]
    assert len(cases) >= 21
    bad = _differences(eng, cases)
    assert not bad, bad


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_every_symbol_at_its_extremes(eng, accepted, frame):
    """every length symbol and every distance symbol the frame's text allows at its first and last value, under the fixed
    codes and under a header of all 286 + 30 lengths"""
    cases = [c for c in accepted if c.frame == frame and c.name in ("every_symbol_extremes", "hlit_286_hdist_30")]
    assert len(cases) == 2
    bad = _differences(eng, cases)
    assert not bad, bad


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_overlap_grid(eng, accepted, frame):
    """WaveSink::copy against the byte-serial copy: every distance 1 .. 69 and 127 .. 129 with lengths around the
    distance and around the wave's width (the large frame: its one member, beyond offset 32 768)"""
    cases = [c for c in accepted if c.frame == frame and c.name.startswith("overlap_grid")]
    assert len(cases) >= (1 if frame == "bgzf64" else 2)
    bad = _differences(eng, cases)
    assert not bad, bad


@pytest.mark.parametrize("frame", ie.FRAMES)
def test_random_members_in_one_call(eng, random_files, frame):
    data, text, index = random_files[frame]
    assert host_gunzip(eng, frame, data) == (text, "")
    got, why = device_gunzip(eng, frame, data)
    assert got == text, why or ie.where_in_file(got, text, index)


def test_refused_cases_are_not_taken_and_leave_nothing_behind(eng, accepted):
    """every refused member comes back not taken with the host model's member and reason -- the one the case was made
    for --, and a good member decoded right after it in the same context gives its text.  The host model refuses each
    before it goes to the device."""
    good = {f: next(c for c in accepted if (c.name, c.frame) == ("hlit_257_hdist_1_after_full", f)) for f in ("plain", "bgzf")}
    bad = []
    for r in ie.refused(chunk_bytes()):
        on_host, why_host = host_gunzip(eng, r.frame, r.data)
        assert on_host is None and why_host.endswith(f"not taken: member {r.member}: {r.reason}"), (r.name, why_host)
        got, why = device_gunzip(eng, r.frame, r.data)
        if got is not None:
            bad.append(f"{r.name} ({r.frame}): taken")
        elif why.split("not taken: ")[-1] != why_host.split("not taken: ")[-1]:
            bad.append(f"{r.name} ({r.frame}): {why!r} on the device, {why_host!r} by the host model")
        g = good[r.frame]
        if device_gunzip(eng, g.frame, g.data) != (g.text, ""):
            bad.append(f"{r.name} ({r.frame}): the good member behind it")
    assert not bad, bad
