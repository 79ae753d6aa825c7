"""The deflate encoder on the GPU (pf_gzip_device, csrc/pf_deflate.hip) on the cases of tests/deflate_cases.py: every
output must decode, with Python's gzip (all members, every CRC32 and ISIZE checked), to the input byte for byte; its
tokens are those of the kernel's documented match rule (tests/deflate_tokens.py: parse_device), its block type the
smallest, its dynamic codes complete, limited and as cheap as Huffman's; the chunks a workgroup encodes one after
the other come out as each does alone."""
import ctypes as C
import gzip
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_tokens as dt  # noqa: E402

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


@pytest.fixture(scope="module")
def audits(eng):
    """every case encoded under each of its flag sets and decoded to tokens, once: name -> (failures, members)"""
    C_ = chunk_bytes()
    return {name: dc.audit(name, data, flagset, lambda d, f: device_gzip(eng, d, f), dt.parse_device, C_)
            for name, data, flagset in dc.cases(C_)}


def test_tokens_block_choice_and_codes_of_every_case(audits):
    """the tokens of every coded block are parse_device's under every block type, none is a match under LITERALS_ONLY;
    the unforced type is the smallest of the three by exact size; every dynamic code is complete, at most 15 bits deep,
    covers exactly the used symbols and costs what Huffman's does unless that is deeper than 15 bits"""
    bad = [b for failures, _ in audits.values() for b in failures]
    assert not bad, (len(bad), bad[:20])


def test_fibonacci_code_is_limited_to_15_bits(audits):
    (m,) = audits["fibonacci"][1][dc.LITERALS_ONLY | dc.DYNAMIC_ONLY]
    ll, _ = dt.histograms(m.tokens)
    assert dt.huffman(ll)[1] >= 17
    assert max(m.ll_len) == 15 and sum(f * n for f, n in zip(ll, m.ll_len)) >= dt.huffman(ll)[0]


def test_every_symbol_comes_from_its_named_case(audits):
    """computed from the kernel's own tokens: each length symbol 258..285 from len<L>, each distance symbol from dist<D>,
    all length symbols in one chunk, and in wide_tokens a token that put_bits spreads over three words"""
    bad = dc.coverage_gaps({name: decoded for name, (_, decoded) in audits.items()}, chunk_bytes())
    assert not bad, bad


def test_chunks_of_one_workgroup_are_encoded_as_each_is_alone(eng):
    """1 100 whole chunks and a ragged tail: more than two chunks for each of the 512 workgroups of a 256-CU part.  Six
    kinds of chunk take turns so that the chunks a workgroup meets one after the other (i, i + grid, ..) differ in kind;
    every member must be, byte for byte, the single member of its chunk's text encoded alone: nothing of a chunk -- the
    match carried past a step, the histograms, the token stream, the member staged where the text goes -- reaches the next."""
    C_ = chunk_bytes()
    kinds = dc.chunk_kinds(C_)
    tail = dc.real_shapes(C_)["kmers_tsv"][:C_ // 3 + 5]
    alone = [device_gzip(eng, text, 0) for _, text, _ in kinds]
    tail_alone = device_gzip(eng, tail, 0)
    for (name, text, btype), member in zip(kinds, alone):
        (m,) = dt.members(member)
        assert m.text == text and btype in (None, m.btype), (name, m.btype)
    assert gzip.decompress(tail_alone) == tail
    order = [(i + i // 512) % len(kinds) for i in range(1100)]
    assert all(order[i] != order[i + 512] for i in range(1100 - 512))
    raw = device_gzip(eng, b"".join(kinds[k][1] for k in order) + tail, 0)
    at, bad = 0, []
    for i, want in enumerate([alone[k] for k in order] + [tail_alone]):
        z = zlib.decompressobj(31)
        piece = raw[at:at + 2 * C_]
        z.decompress(piece)
        assert z.eof, f"member {i} does not end"
        size = len(piece) - len(z.unused_data)
        if raw[at:at + size] != want:
            bad.append((i, "tail" if i == 1100 else kinds[order[i]][0], size, len(want)))
        at += size
    assert at == len(raw)
    assert not bad, (len(bad), bad[:10])
