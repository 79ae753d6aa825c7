"""The hand-out state of the device-written texts, plain and as gzip members: the stream's block in flight across several
ranges, a stream left half way, the mode switched with a stream open, the single-buffer text ended by a stream, an
empty second text of a render, and the places where the one stream's two producers meet (kmers.tsv ranges, pattern-row
slices).  Every case uses the hand-made batch of seam_batch at the smallest budget that works."""
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


# ---- the one stream's two producers, one after (or over) the other.  The pattern ids are the batch's own pool in
# first-seen order, the expected pattern text is the renderer's.
GZ = pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])


def _pool(eng):
    """(the pool's ids in first-seen order, their rows as pf_render_pattern_rows writes them)"""
    _md5, first_seen = eng.export_patterns()
    ids = np.argsort(first_seen, kind="stable").astype(np.uint32)
    return ids, b"".join(eng.render_pattern_rows(ids))


def _rows_begin(eng, ids, slice_bytes):
    total, slices = C.c_uint64(), C.c_uint32()
    rc = eng.L.pf_pattern_rows_stream_begin(eng.ctx, ids.ctypes.data_as(C.c_void_p), len(ids), slice_bytes,
                                            C.byref(total), C.byref(slices))
    return rc, int(total.value), int(slices.value)


def _rows_next(eng):
    ptr, nb = C.c_void_p(), C.c_uint64()
    return eng.L.pf_pattern_rows_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)), int(nb.value)


def _rows(eng, ids, slice_bytes):
    """(text, per block its text bytes, per block its gzip members -- 0 for a block of text) of a whole pattern-row stream"""
    blocks, members = [], []

    def sink(blk):
        raw = bytes(blk.view) if eng.device_gzip else None
        blocks.append(seam_batch.inflate(raw) if eng.device_gzip else bytes(blk))
        members.append(_count_members(raw) if eng.device_gzip else 0)
    text, _handed, slices = eng.stream_pattern_rows(ids, sink, slice_bytes=slice_bytes)
    assert slices == len(blocks) and text == sum(len(b) for b in blocks)
    return b"".join(blocks), [len(b) for b in blocks], members


def _count_members(raw):
    import zlib
    n = 0
    while raw:
        d = zlib.decompressobj(31)
        d.decompress(raw)
        assert d.eof
        raw, n = d.unused_data, n + 1
    return n


@GZ
def test_kmers_tsv_begun_over_a_half_taken_pattern_row_stream(batches, gz):
    from panfeed_amd import _lib
    with _Open(batches[True], True, device_gzip=gz) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        ids, expect = _pool(eng)
        rc, total, slices = _rows_begin(eng, ids, 100)
        assert rc == 0 and total == len(expect) and slices >= 3
        rc, nb = _rows_next(eng)
        assert rc == 0 and nb > 0
        text, _sizes, (n, ranges, _peak) = _stream(eng, o.hb, smallest)      # ends the pattern-row stream, silently
        assert text == o.ek and n == len(o.ek) and ranges > 1
        assert _rows_next(eng)[0] == _lib.ERR_STATE
        assert _rows(eng, ids, 100)[0] == expect


@GZ
def test_pattern_rows_after_an_abandoned_kmers_tsv_stream_with_cuts(batches, gz):
    """The batch is one cluster, so its only cluster end is the text's end, which is no cut inside the text.  The cuts
    given are that end and, so that abandoned cuts would fall inside the pattern rows' slices, every 40th byte of the
    text's first 400: a leaked cut would end a member inside a slice.  Text is cut anywhere, so a plain stream refuses
    cuts (ERR_STATE) and the rest of the case runs without them."""
    from panfeed_amd import _lib
    from test_gpu_pattern_rows_stream import _expected_slices
    with _Open(batches[True], True, device_gzip=gz) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        ids, expect = _pool(eng)
        with eng._target_records(o.hb) as (arr, n):
            total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
            _lib.check(eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, smallest, C.byref(total), C.byref(ranges),
                                                       C.byref(peak)))
            ends = [int(e) for e in eng.target_cluster_ends(o.hb)]
            assert ends == [len(o.ek)] and ranges.value > 1
            cuts = np.array(list(range(40, 440, 40)) + ends, dtype=np.uint64)
            assert eng.L.pf_kmers_tsv_stream_cuts(eng.ctx, cuts.ctypes.data, len(cuts)) == (0 if gz else _lib.ERR_STATE)
            rc, nb = _next(eng)
            assert rc == 0 and nb > 0
        _lib.check(eng.L.pf_set_device_gzip(eng.ctx, int(gz), 0))            # the mode as it is: the stream is abandoned
        assert _next(eng)[0] == _lib.ERR_STATE
        text, sizes, members = _rows(eng, ids, 100)
        assert text == expect
        assert sizes == _expected_slices(expect.splitlines(keepends=True), 100) and len(sizes) >= 3
        assert members == [int(gz)] * len(sizes)


@GZ
def test_refused_pattern_row_begin_leaves_the_open_stream_whole(batches, gz):
    from panfeed_amd import _lib
    with _Open(batches[False], False, device_gzip=gz) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        ids, expect = _pool(eng)
        take = (lambda ptr, nb: seam_batch.inflate(_mem_bytes(ptr, nb))) if gz else _mem_bytes
        with eng._target_records(o.hb) as (arr, n):
            total, ranges, peak = C.c_uint64(), C.c_uint32(), C.c_uint64()
            _lib.check(eng.L.pf_kmers_tsv_stream_begin(eng.ctx, arr, n, smallest, C.byref(total), C.byref(ranges),
                                                       C.byref(peak)))
            ptr, nb = C.c_void_p(), C.c_uint64()
            _lib.check(eng.L.pf_kmers_tsv_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)))
            assert nb.value > 0 and ranges.value > 1
            text = take(ptr, nb.value)
            assert _rows_begin(eng, ids, 100) == (_lib.ERR_STATE, 0, 0)
            assert _rows_next(eng)[0] == _lib.ERR_STATE
            while True:
                _lib.check(eng.L.pf_kmers_tsv_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)))
                if not nb.value:
                    break
                text += take(ptr, nb.value)
        assert text == o.ek
        assert _rows(eng, ids, 100)[0] == expect


def _mem_bytes(ptr, nb):
    from panfeed_amd.engine import _mem
    return bytes(_mem(ptr, nb))


@GZ
def test_single_buffer_text_ends_when_a_pattern_row_stream_begins(batches, gz):
    from panfeed_amd import _lib
    with _Open(batches[True], True, device_gzip=gz) as o:
        eng = o.eng
        ids, expect = _pool(eng)
        assert len(eng.render_targets_device(o.hb)) == len(o.ek)
        assert _chunk(eng, 0) == (0, 1000)
        rc, total, slices = _rows_begin(eng, ids, 100)
        assert rc == 0 and total == len(expect) and slices >= 3
        assert _chunk(eng, 0) == (0, 0)
        assert _chunk(eng, 1)[0] == _lib.ERR_ARG
        text = b""
        while True:
            ptr, nb = C.c_void_p(), C.c_uint64()
            _lib.check(eng.L.pf_pattern_rows_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)))
            if not nb.value:
                break
            text += seam_batch.inflate(_mem_bytes(ptr, nb.value)) if gz else _mem_bytes(ptr, nb.value)
        assert text == expect
        assert bytes(eng.render_targets_device(o.hb)) == o.ek


@GZ
def test_producers_alternate_over_buffers_of_changing_sizes(batches, gz):
    """slices of 100 bytes, ranges of a tile or so, one slice of all rows, one range of all the text: the shared
    buffers are sized anew for every text, smaller and larger than the text before left them"""
    with _Open(batches[False], False, device_gzip=gz) as o:
        eng = o.eng
        smallest = seam_batch.smallest_budget(eng, o.hb)
        ids, expect = _pool(eng)
        text, sizes, _members = _rows(eng, ids, 100)
        assert text == expect and len(sizes) >= 3
        text, _sizes, (n, ranges, _peak) = _stream(eng, o.hb, smallest)
        assert text == o.ek and n == len(o.ek) and ranges > 1
        text, sizes, _members = _rows(eng, ids, 0)
        assert text == expect and sizes == [len(expect)]
        assert bytes(eng.render_targets_device(o.hb)) == o.ek
