"""The stream of pattern rows (pf_pattern_rows_stream_begin / _next, Engine.stream_pattern_rows) against
pf_render_pattern_rows: the same bytes for any list of ids -- first-seen order, reversed, with repeats, one id, none -- at
every slice size (64 MiB: one slice; 1 024 bytes: a few rows a slice, both pinned blocks reused many times, seams between
rows; 100 bytes: less than a row of 70 strains, one row a slice), plain and as gzip members; the slice count and sizes
follow from the row lengths; the state rules (a second begin, a submit in between, an id beyond the pool)."""
import ctypes as C
import gzip

import numpy as np
import pytest

from conftest import all_cases, case_records

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in all_cases()}
SLICES = (0, 1024, 100)
BLOCK = 64 << 20


def _engine(case, **kw):
    from panfeed_amd.engine import Engine
    o = case["opts"]
    eng = Engine(klength=o["klength"], canon=o["canon"], consider_missing=o["consider_missing"], patfilt=o["patfilt"],
                 maf=o["maf"], max_strains=(len(case["all_strains"]) + 31) // 32 * 32, stroi=set(o["stroi"] or ()), **kw)
    for _ in eng.run_stream(case_records(case), batch_clusters=3, defer_patterns=True, device_text=True):
        pass
    return eng


def _orders(eng):
    """(name, ids) for the id lists of a case, and the pool's size"""
    md5, fs = eng.export_patterns()
    first_seen = np.argsort(fs, kind="stable").astype(np.uint32)
    n = len(first_seen)
    assert n == eng.pattern_count() and n > 20
    repeats = np.concatenate([first_seen[:7], first_seen[:7], first_seen[3:4].repeat(5), first_seen[::-1][:9]])
    return [("first_seen", first_seen), ("reversed", first_seen[::-1].copy()), ("repeats", repeats),
            ("single", first_seen[n // 2:n // 2 + 1]), ("none", first_seen[:0])], n


def _expected_slices(rows, slice_bytes):
    """sizes of the slices of `rows` (their bytes, in order): cut between rows, at most cap bytes, or one row"""
    cap = slice_bytes if 0 < slice_bytes < BLOCK else BLOCK
    sizes = []
    for r in rows:
        if sizes and sizes[-1] + len(r) <= cap:
            sizes[-1] += len(r)
        else:
            sizes.append(len(r))
    return sizes


def _gunzip_device(eng, data):
    from panfeed_amd import _lib
    from panfeed_amd.engine import _mem
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(eng.L.pf_gunzip_device(eng.ctx, data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        return taken.value, bytes(_mem(out, n.value))
    finally:
        eng.L.pf_free_text(out)


@pytest.fixture(scope="module", params=["rand70_shuffled", "rand40_shuffled_missing"])
def case(request):
    """(case, the text pf_render_pattern_rows gives for each of its id lists): computed once, from an engine of its own.
    A pattern's id differs from engine to engine, its place in the first-seen order does not: the lists are made of
    places, every engine turns them into its ids (`_orders`)."""
    c = CASES[request.param]
    eng = _engine(c)
    try:
        orders, n = _orders(eng)
        texts = {name: b"".join(eng.render_pattern_rows(ids)) for name, ids in orders}
    finally:
        eng.close()
    # the rendered rows are the reference's (first-seen order is the file's)
    body = c["expect"]["hashes_to_patterns.tsv"].split("\n", 1)[1].encode()
    assert texts["first_seen"] == body
    if c["opts"]["consider_missing"]:
        assert b"\t\t" in body                       # rows with NaN cells
    return c, texts


def test_stream_equals_render(case):
    c, texts = case
    eng = _engine(c)
    try:
        orders, _ = _orders(eng)
        for name, ids in orders:
            rows = texts[name].splitlines(keepends=True)
            for sb in SLICES:
                blocks = []
                text, handed, slices = eng.stream_pattern_rows(ids, lambda b: blocks.append(bytes(b)), slice_bytes=sb)
                assert b"".join(blocks) == texts[name], (name, sb)
                assert [len(b) for b in blocks] == _expected_slices(rows, sb), (name, sb)
                assert slices == len(blocks) and text == handed == len(texts[name]), (name, sb)
        assert len(_expected_slices(texts["first_seen"].splitlines(keepends=True), 1024)) > 4
        assert b"".join(eng.render_pattern_rows(orders[0][1])) == texts["first_seen"]        # the renderer still works
    finally:
        eng.close()


def test_stream_as_gzip_members(case):
    from panfeed_amd.engine import GzipMembers
    c, texts = case
    eng = _engine(c, device_gzip=True)
    try:
        orders, _ = _orders(eng)
        for name, ids in orders:
            rows = texts[name].splitlines(keepends=True)
            for sb in SLICES:
                blocks = []

                def sink(b):
                    assert isinstance(b, GzipMembers) and b.text_bytes is None
                    blocks.append(bytes(b.view))
                text, handed, slices = eng.stream_pattern_rows(ids, sink, slice_bytes=sb)
                data = b"".join(blocks)
                assert gzip.decompress(data) == texts[name] if data else texts[name] == b"", (name, sb)
                assert [len(gzip.decompress(b)) for b in blocks] == _expected_slices(rows, sb), (name, sb)
                assert text == len(texts[name]) and handed == len(data) and slices == len(blocks), (name, sb)
                taken, got = _gunzip_device(eng, data)
                assert taken == 1 and got == texts[name], (name, sb)
    finally:
        eng.close()


def test_state_rules(case):
    from panfeed_amd import _lib
    c, texts = case
    eng = _engine(c)
    try:
        orders, _ = _orders(eng)
        ids = np.ascontiguousarray(orders[0][1], dtype=np.uint32)
        n = eng.pattern_count()
        with pytest.raises(_lib.PanfeedHipError) as e:
            eng.stream_pattern_rows(np.array([0, n], dtype=np.uint32), lambda b: None)
        assert e.value.status == _lib.ERR_ARG

        def begin():
            total, slices = C.c_uint64(), C.c_uint32()
            rc = eng.L.pf_pattern_rows_stream_begin(eng.ctx, ids.ctypes.data_as(C.c_void_p), len(ids), 1024,
                                                    C.byref(total), C.byref(slices))
            return rc, total.value, slices.value

        def nxt():
            ptr, nb = C.c_void_p(), C.c_uint64()
            return eng.L.pf_pattern_rows_stream_next(eng.ctx, C.byref(ptr), C.byref(nb)), nb.value
        # a second begin before the first stream's end
        rc, total, slices = begin()
        assert rc == 0 and total == len(texts["first_seen"]) and slices > 4
        rc, got = nxt()
        assert rc == 0 and 0 < got <= 1024
        assert begin()[0] == _lib.ERR_STATE
        while True:                                   # the first stream is still whole: to its end
            rc, nb = nxt()
            assert rc == 0
            if not nb:
                break
            got += nb
        assert got == total
        assert nxt()[0] == _lib.ERR_STATE             # over: no stream is open
        # a submit in between ends the stream
        assert begin()[0] == 0 and nxt()[0] == 0
        eng.run(case_records(c)[:1])
        assert nxt()[0] == _lib.ERR_STATE
        # and the context streams again afterwards (the pool has grown by what that cluster added, if anything)
        blocks = []
        eng.stream_pattern_rows(ids, lambda b: blocks.append(bytes(b)), slice_bytes=1024)
        assert b"".join(blocks) == texts["first_seen"]
        # pf_reset_patterns empties the pool the rows were measured in: it ends the stream, and no id is left
        assert begin()[0] == 0 and nxt()[0] == 0
        _lib.check(eng.L.pf_reset_patterns(eng.ctx))
        assert nxt()[0] == _lib.ERR_STATE
        assert begin()[0] == _lib.ERR_ARG
    finally:
        eng.close()
