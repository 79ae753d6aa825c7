"""The deflate encoder on the GPU (pf_gzip_device, csrc/pf_deflate.hip) on the cases of tests/deflate_cases.py: every
output must decode, with Python's gzip (all members, every CRC32 and ISIZE checked), to the input byte for byte."""
import ctypes as C
import gzip
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


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


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def test_chunk_size():
    assert 8 << 10 <= chunk_bytes() <= 64 << 10


def test_every_case_decodes_to_the_input(eng):
    C_ = chunk_bytes()
    bad = []
    for name, data, flags in dc.flat_cases(C_):
        members = device_gzip(eng, data, flags)
        try:
            dc.check_members(data, members, C_)
            if name.startswith("incompressible"):
                assert len(members) <= dc.incompressible_cap(len(data), C_)
        except Exception as e:      # noqa: BLE001  (every failing case is named, not only the first)
            bad.append((name, type(e).__name__, str(e)[:80]))
    assert not bad, bad


@pytest.mark.parametrize("shape", ["kmers_to_hashes", "hashes_to_patterns", "kmers_tsv"])
def test_same_text_gives_the_same_bytes(eng, shape):
    text = dc.real_shapes(chunk_bytes())[shape]
    one, two = device_gzip(eng, text, 0), device_gzip(eng, text, 0)
    assert one == two
    assert gzip.decompress(one) == text
    print(f"{shape}: {len(text)} bytes of text -> {len(one)} ({len(text) / len(one):.2f}x)")
    assert len(one) < len(text)


def test_one_product_block_and_a_byte(eng):
    """64 MiB + 1 byte, the block size the product encodes at a time: two launches, the second of one byte"""
    shapes = dc.real_shapes(chunk_bytes())
    unit = shapes["kmers_to_hashes"] + shapes["hashes_to_patterns"] + shapes["kmers_tsv"]
    n = (64 << 20) + 1
    text = (unit * (n // len(unit) + 1))[:n]
    members = device_gzip(eng, text, 0)
    assert gzip.decompress(members) == text
