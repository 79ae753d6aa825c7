"""The segmented device gzip (pf_gzip_device_segments, csrc/pf_deflate.hip): members that end wherever the caller says a
segment ends.  Over the edge shapes of tests/deflate_segments.py and under every flag set: the members of segment i are,
byte for byte, what pf_gzip_device gives for that segment's text alone (the same kernel on an aligned upload -- so nothing
of the text behind a short chunk, and nothing of the way an unaligned chunk is staged, reaches the member); the whole
decodes to the text; two calls give the same bytes; the device decoder takes the output."""
import ctypes as C
import gzip
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_segments as ds  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = {"product": 0, "fixed": 1, "dynamic": 2, "literals": 4}


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def device_gzip(eng, data, flags):
    from panfeed_amd import _lib
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(eng.L.pf_gzip_device(eng.ctx, data, len(data), flags, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        eng.L.pf_free_text(out)


def device_gunzip(eng, members):
    from panfeed_amd import _lib
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(eng.L.pf_gunzip_device(eng.ctx, members, len(members), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        return taken.value, (C.string_at(out, n.value) if n.value else b"")
    finally:
        eng.L.pf_free_text(out)


def test_flags_are_the_librarys():
    from panfeed_amd import _lib
    assert (FLAGS["fixed"], FLAGS["dynamic"], FLAGS["literals"]) == (_lib.GZ_FIXED_ONLY, _lib.GZ_DYNAMIC_ONLY, _lib.GZ_LITERALS_ONLY)


def test_the_shapes_start_at_every_residue():
    starts = set()
    for lengths in ds.shapes(ds.chunk_bytes()).values():
        ends = ds.ends_of(lengths).tolist()
        starts |= {int(s) % 4 for s, n in zip([0] + ends[:-1], lengths) if n}
    assert starts == {0, 1, 2, 3}


@pytest.mark.parametrize("flags", sorted(FLAGS), ids=str)
@pytest.mark.parametrize("shape", sorted(ds.shapes(32768)), ids=str)
def test_segments_equal_their_texts_alone(eng, shape, flags):
    f = FLAGS[flags]
    lengths = ds.shapes(ds.chunk_bytes())[shape]
    ends = ds.ends_of(lengths)
    text = ds.text_of(int(ends[-1]))
    members, member_end = ds.device_segments(eng, text, ends, f)
    assert member_end[-1] == len(members)
    at = m_at = 0
    for n, e, me in zip(lengths, ends.tolist(), member_end):
        piece = text[at:e]
        assert len(piece) == n
        assert members[m_at:me] == device_gzip(eng, piece, f), (shape, flags, at, n)
        at, m_at = e, me
    assert gzip.decompress(members) == text if text else members == b""
    again, again_end = ds.device_segments(eng, text, ends, f)
    assert again == members and again_end == member_end
    taken, back = device_gunzip(eng, members)
    assert taken == 1 and back == text


def test_every_small_segment_is_a_file_of_its_own(eng):
    """2 100 segments of 40 bytes -- more chunks than a launch takes: every piece is a complete gzip file of its text"""
    lengths = ds.shapes(ds.chunk_bytes())["many_small"]
    ends = ds.ends_of(lengths)
    text = ds.text_of(int(ends[-1]))
    members, member_end = ds.device_segments(eng, text, ends, 0)
    at = m_at = 0
    for e, me in zip(ends.tolist(), member_end):
        assert gzip.decompress(members[m_at:me]) == text[at:e]
        at, m_at = e, me


def test_no_segment_and_refusals(eng):
    from panfeed_amd import _lib
    import numpy as np
    assert ds.device_segments(eng, b"", np.zeros(0, dtype=np.uint64)) == (b"", [])
    for ends in ([5, 3, 10], [4, 9], [4, 11]):
        with pytest.raises(_lib.PanfeedHipError) as e:
            ds.device_segments(eng, b"0123456789", np.asarray(ends, dtype=np.uint64))
        assert e.value.status == _lib.ERR_ARG
