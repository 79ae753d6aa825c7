"""Shared by the tests of the segmented gzip (test_deflate_segments_host.py, test_gpu_deflate_segments.py): the texts, the
edge shapes of the segment list, the ctypes calls."""
import ctypes as C
import random

import numpy as np


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def shapes(c):
    """name -> segment lengths: nothing, one byte, the chunk's size and its neighbours, empty segments before, between and
    behind the others, and more chunks than a launch takes (64 MiB / c of them)"""
    return {
        "empty": [0],
        "one_byte": [1],
        "chunk": [c],
        "chunk_and_a_byte": [c + 1],
        "mixed": [0, 5, 0, 0, c - 1, 1, c, c + 1, 2 * c + 3, 0],
        "many_small": [40] * 2100,
        "residues": [7, 6, 5, 9, 3 * c // 2 + 1, 11, 100],       # starts at 0, 7, 13, 18, 27: every residue modulo 4
    }


def text_of(n, seed=7):
    """n bytes: TSV-like rows (a k-mer, a cluster name, a hash: what kmers_to_hashes.tsv looks like), with 4 KiB of random
    bytes in the middle of the first chunk's worth, which no code shortens: stored blocks occur"""
    rng = random.Random(seed)
    rows = []
    size = 0
    while size < n + 64:
        row = "%s\tgroup_%d\t%s\n" % ("".join(rng.choice("ACGT") for _ in range(21)), rng.randrange(40),
                                       "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEF0123456789+/") for _ in range(22)))
        rows.append(row)
        size += len(row)
    text = bytearray("".join(rows).encode()[:n])
    noise = bytes(rng.getrandbits(8) for _ in range(4096))
    at = min(len(text), 9001)          # (odd: the noise starts off a word boundary)
    text[at:at + len(noise)] = noise[:max(0, len(text) - at)]
    return bytes(text[:n])


def ends_of(lengths):
    return np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64) if len(lengths) else np.zeros(0, dtype=np.uint64)


def _call(fn, head, data, ends, flags):
    """(members, member_end) of a pf_gzip_*_segments call; raises panfeed_amd._lib.PanfeedHipError on a refusal"""
    from panfeed_amd import _lib
    L = _lib.load()
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    member_end = np.zeros(max(len(ends), 1), dtype=np.uint64)
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(fn(*head, data, len(data), ends.ctypes.data if len(ends) else None, len(ends), flags, C.byref(out), C.byref(n),
                  member_end.ctypes.data if len(ends) else None))
    try:
        return (C.string_at(out, n.value) if n.value else b""), member_end[:len(ends)].tolist()
    finally:
        L.pf_free_text(out)


def host_segments(data, ends, flags=0):
    from panfeed_amd import _lib
    return _call(_lib.load().pf_gzip_host_model_segments, (), data, ends, flags)


def device_segments(eng, data, ends, flags=0):
    return _call(eng.L.pf_gzip_device_segments, (eng.ctx,), data, ends, flags)
