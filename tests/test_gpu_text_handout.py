"""The hand-out state of the device-written texts, plain and as gzip members: the stream's block in flight across several
ranges, a stream left half way, the mode switched with a stream open, the single-buffer text ended by a stream, and an
empty second text of a render.  Every case uses the hand-made batch of seam_batch at the smallest budget that works."""
import ctypes as C

import numpy as np
import pytest

import seam_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    return {canon: seam_batch.build(canon) for canon in (True, False)}


class _Open:
    """an engine with the batch submitted: .eng, .hb, .ek (the oracle's kmers.tsv bytes)"""

    def __init__(self, batch, canon, **kw):
        from panfeed_amd.engine import Engine
        from panfeed_amd.packing import build_batch_native
        recs, stroi, self.ek = batch
        self.eng = Engine(klength=seam_batch.K, canon=canon, max_strains=32, stroi=stroi, **kw)
        try:
            self.hb = build_batch_native(recs, seam_batch.K, canon, self.eng.W, stroi=stroi, first_ordinal=0)
            self.eng.submit_host_batch(self.hb)
        except Exception:
            self.eng.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()


def _stream(eng, hb, budget):
    """(text, blocks' sizes, (bytes, ranges, peak)) of a whole stream; gzip blocks inflated member by member"""
    from panfeed_amd.engine import GzipMembers
    text, sizes = bytearray(), []

    def sink(blk):
        assert isinstance(blk, GzipMembers) == eng.device_gzip
        sizes.append(len(blk))
        text.extend(seam_batch.inflate(blk.view) if eng.device_gzip else blk)
    res = eng.stream_targets_device(hb, sink, budget=budget)
    return bytes(text), sizes, res


def _begin_and_take_one(eng, hb, budget):
    """a stream begun and left after its first block: (status of begin, status of next, the block's bytes)"""
    with eng._target_records(hb) as (arr, n):
        total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
        rc0 = eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, budget, C.byref(total), C.byref(ranges), C.byref(peak))
        rc1, nb = _next(eng)
    assert rc0 == 0 and rc1 == 0 and nb > 0 and ranges.value > 1
    return nb


def _next(eng):
    ptr, nb = C.c_void_p(), C.c_uint64()
    return eng.L.pf_kmers_tsv_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)), int(nb.value)


def _chunk(eng, offset, max_bytes=1000):
    ptr, nb = C.c_void_p(), C.c_uint64()
    return eng.L.pf_device_text_chunk(eng.ctx, offset, max_bytes, C.byref(ptr), C.byref(nb)), int(nb.value)


def _addr(view):
    return np.frombuffer(view, dtype=np.uint8).ctypes.data


def _texts(pair):
    return tuple(bytes(x) for x in pair)


@pytest.mark.parametrize("canon", [True, False], ids=["canonical", "non_canonical"])
def test_gzip_stream_over_several_ranges(batches, canon):
    with _Open(batches[canon], canon, device_gzip=True) as o:
        smallest = seam_batch.smallest_budget(o.eng, o.hb)
        text, sizes, (n, ranges, _peak) = _stream(o.eng, o.hb, smallest)
        assert text == o.ek
        assert ranges > 1
        assert n == len(o.ek)
        assert o.eng.stream_compressed == sum(sizes)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
def test_abandoned_stream(batches, gz):
    with _Open(batches[True], True, device_gzip=gz) as o:
        smallest = seam_batch.smallest_budget(o.eng, o.hb)
        before = _texts(o.eng.render_device(o.hb))
        _begin_and_take_one(o.eng, o.hb, smallest)
        text, _sizes, (n, ranges, _peak) = _stream(o.eng, o.hb, smallest)
        assert text == o.ek and n == len(o.ek) and ranges > 1
        assert _texts(o.eng.render_device(o.hb)) == before


def test_mode_switch_with_a_stream_open(batches):
    from panfeed_amd import _lib
    with _Open(batches[False], False) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        _begin_and_take_one(eng, o.hb, smallest)
        _lib.check(eng.L.pf_set_device_gzip(eng.ctx, 1, 0))
        eng.device_gzip = True
        assert _next(eng)[0] == _lib.ERR_STATE
        text, _sizes, (n, ranges, _peak) = _stream(eng, o.hb, smallest)
        assert text == o.ek and n == len(o.ek) and ranges > 1
        _begin_and_take_one(eng, o.hb, smallest)
        _lib.check(eng.L.pf_set_device_gzip(eng.ctx, 0, 0))
        eng.device_gzip = False
        assert _next(eng)[0] == _lib.ERR_STATE
        text, _sizes, (n, ranges, _peak) = _stream(eng, o.hb, smallest)
        assert text == o.ek and n == len(o.ek) and ranges > 1


def test_single_buffer_text_ends_when_a_stream_begins(batches):
    from panfeed_amd import _lib
    with _Open(batches[True], True) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        text = eng.render_targets_device(o.hb)
        assert len(text) == len(o.ek)
        assert _chunk(eng, 0) == (0, 1000)
        with eng._target_records(o.hb) as (arr, n):
            total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
            _lib.check(eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, smallest, C.byref(total), C.byref(ranges),
                                                       C.byref(peak)))
            assert _chunk(eng, 0) == (0, 0)
            assert _chunk(eng, 1)[0] == _lib.ERR_ARG
            streamed = 0
            while True:
                rc, nb = _next(eng)
                assert rc == 0
                if not nb:
                    break
                streamed += nb
        assert streamed == total.value == len(o.ek)
        assert bytes(eng.render_targets_device(o.hb)) == o.ek


def test_empty_second_text_under_gzip(batches):
    from panfeed_amd.engine import GzipMembers
    with _Open(batches[False], False) as o:
        plain = _texts(o.eng.render_device(o.hb))
    assert plain[0] and plain[1]
    with _Open(batches[False], False, device_gzip=True) as o:
        kh, hp = o.eng.render_device(o.hb, defer_patterns=True)
        assert isinstance(hp, GzipMembers) and len(hp) == 0 and hp.text_bytes == 0
        assert isinstance(kh, GzipMembers) and kh.text_bytes == len(plain[0])
        assert seam_batch.inflate(kh.view) == plain[0]
        # both texts present: two views of one pinned block, the second behind the first
        kh, hp = o.eng.render_device(o.hb)
        assert seam_batch.inflate(kh.view) == plain[0] and seam_batch.inflate(hp.view) == plain[1]
        assert _addr(kh.view) + len(kh) <= _addr(hp.view)
