"""The block-scale cases of tests/block_scale.py, held to their own claims without a GPU: the mirrored constants equal the
source, every case stands on the quantity it claims -- asserted from its bytes, so that a case cut below its constant
fails here --, the construction shortcut equals the models on a prefix of every table and on a period of every periodic
file, and the member files are what they claim by gzip, by the BGZF walker and by the decoder's host model."""
import ctypes as C
import gzip
import os
import struct
import sys
from itertools import accumulate

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
import bgzf_cases as bc  # noqa: E402
import block_scale as bs  # noqa: E402
import join_tables as jt  # noqa: E402
import text_tables as tt  # noqa: E402

from panfeed_amd import _lib, downstream  # noqa: E402

PREFIX = 5000                     # rows of every table the models run over
_CONTROL = bytes(c for c in range(32) if c not in (9, 10)) + b'"'


def chunk_bytes():
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def test_mirrored_constants_equal_the_source():
    src, gone = bs.source_constants()
    assert set(src) == set(bs.MIRROR)
    wrong = {k: (bs.MIRROR[k], src[k]) for k in bs.MIRROR if bs.MIRROR[k] != src[k]}
    assert not wrong, f"mirrored constants differ from the source (mirror, source): {wrong}"
    assert not gone, "expressions the cases rest on are no longer in the source:\n" + "\n".join(gone)


def test_derived_quantities():
    assert bs.TILE == 65536 and bs.SWEEP == 524288
    assert bs.max_members(chunk_bytes()) == bs.MAX_TEXT // chunk_bytes() >= 2
    assert downstream.BLOCK_BYTES == bs.MAX_TEXT                                  # a block of the tools is a call of the feed
    assert bs.MAX_TEXT // bs.M["BGZF_MAX_TEXT"] == 4096 and bs.row_tiles(downstream.BLOCK_BYTES) == 4096
    assert [bs.row_tiles(n) for n in (0, 1, bs.TILE, bs.TILE + 1, 256 * bs.TILE, 256 * bs.TILE + 1)] == [0, 1, 1, 2, 256, 257]
    assert [bs.tiles_per_thread(t) for t in (1, 256, 257, 512, 513, 4096)] == [1, 1, 2, 2, 3, 16]
    assert bs.GZ_BLOCK == 2 * bs.ROW_PIECE and bs.GZ_BLOCK % chunk_bytes() == 0


# ------------------------------------------------------------------------------------------------ associations tables
def _af_rows(case):
    """(the data rows, [(start, end)] of each in the scanned text, its newline included)"""
    body = case.text[len(at.HEADER):]
    assert case.text.startswith(at.HEADER) and body.endswith(b"\n")
    rows = body[:-1].split(b"\n")
    ends = list(accumulate(len(r) + 1 for r in rows))
    return rows, list(zip([0] + ends[:-1], ends)), body


def _af_holds(case):
    """what every associations case claims: rows that differ from one another, no flagged row, the kept lines those of
    `keep`, and the models' answer on the first rows"""
    rows, spans, body = _af_rows(case)
    assert len(rows) == case.rows == len(case.keep) and len(set(rows)) == len(rows)
    assert body.count(b"\t") == 7 * len(rows) and len(body.translate(None, _CONTROL)) == len(body)
    assert max(e - b for b, e in spans) < 200 and case.flags == 0
    assert case.n_kept == sum(case.keep) and case.kept == b"".join(r + b"\n" for r, k in zip(rows, case.keep) if k)
    m = at.scan(at.HEADER + b"".join(r + b"\n" for r in rows[:PREFIX]), at.PVALUE_FIELD, case.thr)
    assert m.rows == PREFIX and m.flags == 0 and 0 < m.n_kept == sum(case.keep[:PREFIX])
    assert case.kept.startswith(m.kept) and case.kept[len(m.kept):len(m.kept) + 1] in (b"H", b"")
    assert m.classes == case.classes
    return rows, spans, body


@pytest.fixture(scope="module")
def tiles_257():
    return bs.af_tiles_257()


def test_af_tiles_257(tiles_257):
    case = tiles_257
    rows, spans, body = _af_holds(case)
    t255, t256 = 255 * bs.TILE, 256 * bs.TILE
    assert t256 + 200 <= len(body) <= t256 + 1000
    assert bs.row_tiles(len(body)) == 257 and bs.tiles_per_thread(257) == 2
    kept = [s for s, k in zip(spans, case.keep) if k]
    assert any(b < t255 < e for b, e in kept)                  # a kept row across the start of tile 255
    assert any(b < t256 < e for b, e in kept)                  # another across the start of tile 256
    last_tile = [(s, k) for s, k in zip(spans, case.keep) if s[0] >= t256]
    assert len(last_tile) in (2, 3) and all(k for _, k in last_tile)
    assert case.keep[0] and case.keep[-1]
    assert len(kept) * 1000 < len(rows)                        # sparse: the forced places are not hidden among others
    # kept rows in tiles far apart, so that a wrong prefix anywhere moves one of them
    assert len({b // bs.TILE for b, _ in kept}) >= 40


@pytest.fixture(scope="module")
def sweep_and_pieces():
    return bs.af_sweep_and_pieces()


def test_af_sweep_and_pieces(sweep_and_pieces):
    case = sweep_and_pieces
    rows, spans, body = _af_holds(case)
    assert case.n_kept >= bs.SWEEP + 17
    assert len(case.kept) >= 2 * bs.ROW_PIECE + 1 and len(case.kept) < 3 * bs.ROW_PIECE
    assert all(k == (i % 7 != 3) for i, k in enumerate(case.keep))
    tiles = bs.row_tiles(len(body))
    assert tiles > 1000 and bs.tiles_per_thread(tiles) == 5 and tiles % 5 != 0
    assert len(case.text) <= downstream.BLOCK_BYTES            # one block of the plain route


# ------------------------------------------------------------------------------------------------ kmers.tsv tables
def _kj_holds(case):
    rows = case.body[:-1].split(b"\n")
    assert case.body.endswith(b"\n") and len(case.header + case.body) <= downstream.BLOCK_BYTES
    sel = [r for r in rows if r.startswith(b"sel\t")]
    assert len(sel) == case.rows and case.want[0].count(b"\n") == case.want[1].count(b"\n") == case.rows
    assert case.want[2].count(b"\n") == case.rows - case.unmatched
    head = rows[:PREFIX]
    texts = [dict(zip(case.keys, t)) for t in (case.text0, case.text1)]
    for mode in (0, 1):
        m = jt.join_rows(head, {b"sel"}, texts[mode], case.empty)
        assert m and case.want[mode].startswith(m) and case.want[mode][len(m):len(m) + 4] == b"sel\t"
    m = jt.kept_rows(head, {b"sel"}, set(case.keys))
    assert m and case.want[2].startswith(m)
    plan = jt.survey(head, [{b"sel"}, {b"oth"}], set(case.keys))
    assert plan[0]["flags"] == 0 and plan[1]["flags"] == 0 and plan[0]["rows"] == sum(r.startswith(b"sel\t") for r in head)
    return rows, sel


@pytest.fixture(scope="module")
def rows_sweep():
    return bs.kj_rows_sweep()


def test_kj_rows_sweep(rows_sweep):
    case = rows_sweep
    rows, sel = _kj_holds(case)
    assert case.rows >= bs.SWEEP + 17 and bs.row_tiles(len(case.body)) > 256
    assert all(r.startswith(b"sel\t") == (i % 5 != 4) for i, r in enumerate(rows))
    others = {r.split(b"\t", 1)[0] for r in rows[4::5]}
    assert others == {b"oth", b"zz"}
    assert case.unmatched in (case.rows // 2, case.rows - case.rows // 2)          # half of the bunch's k-mers have a key
    assert (case.text0, case.text1, case.empty) == ([b"t0"], [b"t1.0"], b"")
    assert 0 < len(case.want[2]) < len(case.want[0]) < len(case.want[1])
    assert any(r.endswith(b"\tACG") for r in rows[4::5])       # the key's k-mer under another cluster: no key


def test_kj_long_texts():
    case = bs.kj_long_texts()
    _kj_holds(case)
    assert case.rows == 20000 and case.unmatched == 0
    assert (len(case.text0[0]), len(case.text1[0])) == (3500, 3501)
    for mode in (0, 1):
        assert len(case.want[mode]) >= bs.GZ_BLOCK + 1                             # two slices of the encoder
        assert len(case.want[mode]) > 2 * bs.ROW_PIECE                              # three pieces of the hand-out
    # a row's output lies across byte BLOCK: the slices' seam is inside a row
    assert case.want[0][bs.GZ_BLOCK - 1:bs.GZ_BLOCK] != b"\n"


# ------------------------------------------------------------------------------------------------ member files
def _host_model(call, data):
    L = _lib.load()
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(call(data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        assert taken.value, L.pf_last_error().decode()
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def _isizes(data, offsets):
    return [struct.unpack_from("<I", data, end - 4)[0] for end in offsets[1:] + [len(data)]]


@pytest.mark.parametrize("table", ["rf", "af"])
def test_members_over_the_count(table):
    chunk = chunk_bytes()
    mm = bs.max_members(chunk)
    mf = bs.members_over_the_count(table, chunk)
    head = mf.text.index(b"\n") + 1
    assert mf.n_members == 2 * mm + 6 and len(mf.text) == head + (2 * mm + 5) * bs.UNIT
    s1, s2 = bs.count_seams(mf, chunk)
    L = _lib.load()
    for data, offsets, extra in ((mf.plain, bs.plain_offsets(mf.plain), 0), (mf.bgzf, bs.bgzf_offsets(mf.bgzf), 1)):
        assert len(offsets) == mf.n_members + extra
        sizes = _isizes(data, offsets)
        assert sizes[0] == head and sizes[1:mf.n_members] == [bs.UNIT] * (mf.n_members - 1) and sizes[mf.n_members:] == [0] * extra
        assert gzip.decompress(data) == mf.text
        # the offsets of members MAX_MEMBERS and 2 * MAX_MEMBERS: what a first and a second call leave
        assert gzip.decompress(data[:offsets[mm]]) == mf.text[:s1]
        assert gzip.decompress(data[offsets[mm]:offsets[2 * mm]]) == mf.text[s1:s2]
        assert len(offsets) - 2 * mm == 6 + extra and gzip.decompress(data[offsets[2 * mm]:]) == mf.text[s2:]
    assert bc.walked_text(mf.bgzf[:bs.bgzf_offsets(mf.bgzf)[3]] + bc.EOF) == mf.text[:head + 2 * bs.UNIT]
    assert _host_model(L.pf_gunzip_host_model, mf.plain) == mf.text
    assert _host_model(L.pf_gunzip_host_model_bgzf, mf.bgzf) == mf.text
    # both call seams inside a line; most lines across a member seam
    assert all(b"\n" not in mf.text[s - 1:s + 1] for s in (s1, s2))
    ends = list(accumulate(len(ln) + 1 for ln in mf.text[head:-1].split(b"\n")))
    across = sum((b // bs.UNIT) != ((e - 1) // bs.UNIT) for b, e in zip([0] + ends[:-1], ends))
    assert across * 4 > len(ends) * 3
    # the expectation holds rows of every call: the last line starts behind the second seam and is kept
    last = mf.text[mf.text.rfind(b"\n", 0, -1) + 1:]
    assert len(mf.text) - len(last) > s2
    if table == "rf":
        for first in (True, False):
            want = bs.rf_expect(mf.text, first)
            assert want.endswith(last) and tt.filter_rows(mf.text[head:s1], bs.RF_KEYS, first) and want != bs.rf_expect(mf.text, not first)
    else:
        want = bs.af_expect(mf.text)
        assert want.kept.endswith(last) and 0 < want.n_kept < want.rows and want.flags == 0


@pytest.mark.parametrize("table", ["rf", "af"])
def test_members_over_the_text(table):
    u, data = bs.members_over_the_text(table)
    size = bs.M["BGZF_MAX_TEXT"]
    offsets = bs.bgzf_offsets(data)
    assert len(offsets) == 2 * bs.PERIODS + 2 == 4098                              # 4 097 members of text and the end marker
    assert _isizes(data, offsets) == [size] * 4097 + [0]
    assert 4096 * size == bs.MAX_TEXT and 4097 * size == bs.MAX_TEXT + 65536       # a first call takes members 0 .. 4 095
    assert [t for _, _, t in bc.walk(data[:offsets[3]] + bc.EOF)] == [u.C, u.A, u.B, b""]
    assert data[offsets[1]:offsets[4097]] == data[offsets[1]:offsets[3]] * bs.PERIODS and data[offsets[4097]:] == bc.EOF
    assert data[offsets[4095]:offsets[4096]] == bc.member(u.A) and data[offsets[4096]:offsets[4097]] == bc.member(u.B)
    assert 20 << 20 < len(data) < 64 << 20
    # a line start strictly inside the straddled members, and the line across their seam is the one the filter keeps
    assert 0 < u.A.rfind(b"\n") + 1 < size and not u.A.endswith(b"\n") and 0 < u.B.find(b"\n") + 1 < size
    assert u.A[u.A.rfind(b"\n") + 1:] + u.B[:u.B.find(b"\n") + 1] == u.straddler
    want = bs.over_the_text_expect(u)
    two = u.C + (u.A + u.B) * 2
    if table == "rf":
        for first in (True, False):
            ab = tt.filter_rows(u.A + u.B, bs.RF_KEYS, first)
            assert ab.count(u.straddler) == 1 and u.straddler not in tt.filter_rows(u.A[:u.A.rfind(b"\n") + 1], bs.RF_KEYS, first)
            assert bs.rf_expect(two, first) == bs.rf_expect(u.C, first) + 2 * ab
            assert want[first].count(u.straddler) == bs.PERIODS and 1 << 20 < len(want[first]) < 16 << 20
        assert want[True] != want[False]
    else:
        c, ab, m = bs.af_expect(u.C), bs.af_expect(at.HEADER + u.A + u.B), bs.af_expect(two)
        assert ab.kept.count(u.straddler) == 1
        assert (m.kept, m.rows, m.n_kept, m.flags) == (c.kept + 2 * ab.kept, c.rows + 2 * ab.rows, c.n_kept + 2 * ab.n_kept, 0)
        assert m.classes == want.classes and want.flags == 0
        assert want.kept.count(u.straddler) == bs.PERIODS and 1 << 20 < len(want.kept) < 16 << 20
        assert want.rows == want.kept.count(b"\n") + (want.rows - want.n_kept) and want.n_kept == want.kept.count(b"\n")
