"""The downstream text path at the product's block size (tests/block_scale.py; tests/test_block_scale.py holds the cases to
their claims): the row pack's tile sums past one tile a thread and its writer past one sweep of its grid, the hand-out
past two pieces, the join's gzip route past one encoder slice, and the device text feed past the members and past the
text bytes one call takes -- each against an expectation known by construction, never one from the device route."""
import ctypes as C
import os
import struct
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
import block_scale as bs  # noqa: E402
import seam_batch  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chunk(eng):
    return int(eng.L.pf_gzip_device_chunk_bytes())


# ------------------------------------------------------------------------------------------------ the associations filter
def _af_pass(path, case):
    from panfeed_amd.downstream import AssocFilter
    f = AssocFilter(at.PVALUE_FIELD, len(at.HEADER.split(b"\t")), case.thr)
    try:
        kept = f.filter_file(str(path))
        return kept, f.columns(), f.stats()
    finally:
        f.close()


def _af_same(got, case):
    kept, cols, st = got
    assert len(kept) == len(case.kept) and kept == case.kept
    assert (cols["classes"], cols["flags"], cols["rows"], cols["kept"]) == (case.classes, case.flags, case.rows, case.n_kept)
    assert st["bytes_scanned"] == len(case.text) - len(at.HEADER) and st["members_inflated"] == 0


def test_af_tiles_257(tmp_path):
    """257 tiles in one block: every thread of row_tiles_kernel sums two tiles, the last working one a single tile, half of
    them none.  The kept rows -- the first, those across the starts of tiles 255 and 256, all of the last tile, the last --
    byte for byte and in order; classes, flags and counters"""
    case = bs.af_tiles_257()
    path = tmp_path / "assoc.tsv"
    path.write_bytes(case.text)
    _af_same(_af_pass(path, case), case)


@pytest.fixture(scope="module")
def sweep_and_pieces():
    return bs.af_sweep_and_pieces()


def test_af_sweep_and_pieces(tmp_path, sweep_and_pieces):
    """over 1 000 tiles (five a thread of row_tiles_kernel, the last thread fewer), more kept rows than one sweep of the
    writer's grid, more kept bytes than two pieces of the hand-out: the plain route, the table in one block"""
    case = sweep_and_pieces
    path = tmp_path / "assoc.tsv"
    path.write_bytes(case.text)
    _af_same(_af_pass(path, case), case)


def test_af_pieces_and_their_lifetime(sweep_and_pieces):
    """pf_assocfilter_next_lines by hand: pieces of ROW_PIECE, ROW_PIECE, the rest and 0 bytes; the third lies in the first
    one's buffer.  A piece is valid until the next call: it holds its bytes right after its call returns and still does
    immediately before the next call is made, after the host has spent the time of a comparison in which the copy of the
    piece behind it lands in the other buffer.  No longer: after the third call has returned, the first piece's bytes have
    changed -- the life "until the call after the next" that the header used to promise did not hold"""
    from panfeed_amd import _lib
    from panfeed_amd.downstream import AssocFilter
    case = sweep_and_pieces
    body, want = case.text[len(at.HEADER):], case.kept
    f = AssocFilter(at.PVALUE_FIELD, len(at.HEADER.split(b"\t")), case.thr)
    try:
        out_bytes, used = C.c_uint64(), C.c_uint64()
        _lib.check(f.L.pf_assocfilter_scan(f.h, body, len(body), C.byref(out_bytes), C.byref(used)))
        assert (out_bytes.value, used.value) == (len(want), len(body))
        pieces, pos, before = [], 0, None             # (pointer, offset in `want`, bytes); the copy of the piece before the held one
        while True:
            if pieces:
                ptr, lo, n = pieces[-1]
                assert C.string_at(ptr, n) == want[lo:lo + n], f"piece {len(pieces) - 1} changed before the next call"
            piece, n = C.c_void_p(), C.c_uint64()
            _lib.check(f.L.pf_assocfilter_next_lines(f.h, C.byref(piece), C.byref(n)))
            if not n.value:
                break
            held = C.string_at(piece.value, n.value)
            assert held == want[pos:pos + n.value], f"piece {len(pieces)} right after its call"
            if before is not None:                                         # the previous piece's comparison, on its copy
                assert before == want[pos - len(before):pos]
            if len(pieces) == 2:                                           # the third call has returned
                first_ptr, _, first_n = pieces[0]
                assert piece.value == first_ptr and pieces[1][0] != first_ptr
                assert C.string_at(first_ptr, n.value) != want[:n.value] and n.value < first_n
            pieces.append((piece.value, pos, n.value))
            pos, before = pos + n.value, held
        assert [n for _, _, n in pieces] == [bs.ROW_PIECE, bs.ROW_PIECE, len(want) - 2 * bs.ROW_PIECE] and pos == len(want)
        cols = f.columns()
        assert (cols["rows"], cols["kept"], cols["flags"]) == (case.rows, case.n_kept, 0)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ the k-mer join
def _join(case, tmp_path):
    from panfeed_amd.downstream import KmerJoin
    path = str(tmp_path / "kmers.tsv")
    with open(path, "wb") as fh:
        fh.write(case.header + case.body)
    return KmerJoin(bs.KJ_CLUSTERS, 2, case.keys, case.text0, case.text1, case.empty), path


def _pieces(kj, path, mode):
    out = []
    kj.join_file(path, 0, mode, lambda piece: out.append(bytes(piece)))
    return out


def test_kj_rows_sweep(tmp_path):
    """bunch 0 has one sweep of the writer's grid and 17 rows, among rows of another bunch and of no bunch, in a block of
    over 256 tiles: the survey's counters, the three modes, the row counts"""
    from panfeed_amd.downstream import KJ_RAW
    case = bs.kj_rows_sweep()
    kj, path = _join(case, tmp_path)
    try:
        plan = kj.survey_file(path)
        assert not kj.members[path]
        assert plan[0] == {"rows": case.rows, "unmatched": case.unmatched, "bytes": (len(case.want[0]), len(case.want[1])), "flags": 0}
        assert plan[1]["flags"] == 0 and plan[1]["rows"] == plan[1]["unmatched"] > 0
        for mode in (0, 1, KJ_RAW):
            got = b"".join(_pieces(kj, path, mode))
            assert len(got) == len(case.want[mode]) and got == case.want[mode], mode
        st = kj.stats()
        assert st["rows_written"] == 2 * case.rows and st["raw_rows"] == case.rows - case.unmatched
        assert st["unmatched_written"] == 2 * case.unmatched and st["hash_rejects"] == 0
    finally:
        kj.close()


def _member_texts(raw):
    """the texts of a run of plain-header gzip members, each inflated by itself: whole members, CRC32 and ISIZE checked"""
    offsets = bs.plain_offsets(raw)
    out = []
    for a, b in zip(offsets, offsets[1:] + [len(raw)]):
        d = zlib.decompressobj(31)
        out.append(d.decompress(raw[a:b]))
        assert d.eof and not d.unused_data and len(out[-1]) == struct.unpack_from("<I", raw, b - 4)[0]
    return out


def test_kj_long_texts(tmp_path, chunk):
    """more text from one join call than PfGzEncoder::BLOCK: the plain hand-out's three pieces; with the gzip switch on,
    whole members of two encoder slices -- none whose text lies across byte BLOCK of the call's text --; and plain text
    again from the same handle with the switch off"""
    case = bs.kj_long_texts()
    kj, path = _join(case, tmp_path)
    try:
        plan = kj.survey_file(path)
        assert plan[0] == {"rows": case.rows, "unmatched": 0, "bytes": (len(case.want[0]), len(case.want[1])), "flags": 0}
        pieces = _pieces(kj, path, 0)
        assert len(pieces) >= 3 and [len(p) for p in pieces[:-1]] == [bs.ROW_PIECE] * (len(pieces) - 1)
        assert b"".join(pieces) == case.want[0]
        del pieces
        kj.set_gzip(True)
        raw = b"".join(_pieces(kj, path, 0))
        assert seam_batch.inflate(raw) == case.want[0]
        texts = _member_texts(raw)
        assert b"".join(texts) == case.want[0]
        ends, total = set(), 0
        for t in texts:
            assert 0 < len(t) <= chunk
            total += len(t)
            ends.add(total)
        assert bs.GZ_BLOCK in ends and total > bs.GZ_BLOCK                      # a member ends the first slice; the next starts the second
        st = kj.stats()
        assert st["gzip_text_bytes"] == len(case.want[0]) and st["gzip_member_bytes"] == len(raw)
        assert st["gzip_device_bytes"] < (256 << 20)
        kj.set_gzip(False)
        assert b"".join(_pieces(kj, path, 1)) == case.want[1]
        assert kj.stats()["gzip_text_bytes"] == len(case.want[0]) and kj.stats()["rows_written"] == 3 * case.rows
    finally:
        kj.close()


# ------------------------------------------------------------------------------------------------ the text feed
def _owner(table, first_field=True):
    from panfeed_amd.downstream import AssocFilter, RowFilter
    if table == "rf":
        return RowFilter(bs.RF_KEYS, first_field)
    return AssocFilter(at.PVALUE_FIELD, len(at.HEADER.split(b"\t")), bs.THR)


def _calls(owner, data, ends):
    """a members pass by hand, every call with `last` set and given all that is left of the file: the calls must use up
    the compressed bytes in front of ends[0], ends[1], ..., the last one the rest.  -> the calls' rows, joined"""
    from panfeed_amd import _lib
    _lib.check(owner._begin_fn(owner.h, 1))
    out, pos = [], 0
    for end in ends:
        rows, used, taken = owner.scan_members(data[pos:], True)
        assert taken and used == end - pos, (pos, used, end)
        out.append(rows)
        pos = end
    assert pos == len(data)
    return b"".join(out)


def _file_pass(owner, path, block_bytes=None):
    got = owner.filter_file(str(path), block_bytes=block_bytes, device_gunzip=True)
    return got[1] if isinstance(got, tuple) else got


def _af_scan_same(owner, m):
    cols = owner.columns()
    assert (cols["classes"], cols["flags"], cols["rows"], cols["kept"]) == (m.classes, m.flags, m.rows, m.n_kept)


def _gunzip(eng, call, data):
    from panfeed_amd import _lib
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(call(eng.ctx, data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        assert taken.value, eng.L.pf_last_error().decode()
        return C.string_at(out, n.value) if n.value else b""
    finally:
        eng.L.pf_free_text(out)


@pytest.mark.parametrize("table", ["rf", "af"])
def test_members_over_the_count(tmp_path, eng, chunk, table):
    """2 * MAX_MEMBERS + 6 members in one read: the feed takes MAX_MEMBERS a call and gives the rest back, with `last` set, in
    both containers; a line lies across either call seam.  Then the whole-file calls, whose loop cuts at the same count"""
    mm = bs.max_members(chunk)
    mf = bs.members_over_the_count(table, chunk)
    want = {first: bs.rf_expect(mf.text, first) for first in (True, False)} if table == "rf" else bs.af_expect(mf.text)
    for name, data, offsets in (("plain", mf.plain, bs.plain_offsets(mf.plain)), ("bgzf", mf.bgzf, bs.bgzf_offsets(mf.bgzf))):
        path = tmp_path / f"{table}.{name}.tsv.gz"
        path.write_bytes(data)
        assert len(data) < 32 << 20                                          # one read of the default block
        for first in (True, False) if table == "rf" else (True,):
            owner = _owner(table, first)
            try:
                got = _file_pass(owner, path)
                st = owner.stats()
                assert (st["members_inflated"], st["text_bytes_inflated"]) == (len(offsets), len(mf.text)), name
                got_by_hand = _calls(owner, data, [offsets[mm], offsets[2 * mm], len(data)])
                assert owner.stats()["members_inflated"] == 2 * len(offsets)
                if table == "rf":
                    assert got == want[first] and got_by_hand == want[first], (name, first)
                else:
                    assert got == want.kept and owner.header == at.HEADER, name
                    assert got_by_hand == want.kept
                    twice = at.Scan(None, want.classes, want.flags, 2 * want.rows, 2 * want.n_kept)
                    _af_scan_same(owner, twice)
            finally:
                owner.close()
    assert _gunzip(eng, eng.L.pf_gunzip_device, mf.plain) == mf.text
    assert _gunzip(eng, eng.L.pf_gunzip_device_bgzf, mf.bgzf) == mf.text


@pytest.fixture(scope="module", params=["rf", "af"])
def over_the_text(request, tmp_path_factory):
    u, data = bs.members_over_the_text(request.param)
    path = tmp_path_factory.mktemp("over_the_text") / f"{request.param}.tsv.gz"
    path.write_bytes(data)
    return u, data, path, bs.over_the_text_expect(u)


def test_members_over_the_text(over_the_text):
    """4 097 BGZF members of 64 KiB of text each, 256 MiB + 64 KiB, read in one block: a call takes the 4 096 members that
    make MAX_TEXT and gives the last one back.  The call seam lies inside a line the filter keeps: it comes out once a period"""
    u, data, path, want = over_the_text
    offsets = bs.bgzf_offsets(data)
    total = (2 * bs.PERIODS + 1) * bs.M["BGZF_MAX_TEXT"]
    for first in (True, False) if u.table == "rf" else (True,):
        owner = _owner(u.table, first)
        try:
            got = _file_pass(owner, path, block_bytes=len(data))
            st = owner.stats()
            assert (st["members_inflated"], st["text_bytes_inflated"]) == (len(offsets), total)
            by_hand = _calls(owner, data, [offsets[4096], len(data)])
            assert owner.stats()["text_bytes_inflated"] == 2 * total
            expect = want[first] if u.table == "rf" else want.kept
            assert len(got) == len(expect) and got == expect, first
            assert by_hand == expect, first
            assert got.count(u.straddler) == bs.PERIODS
            if u.table == "af":
                _af_scan_same(owner, at.Scan(None, want.classes, want.flags, 2 * want.rows, 2 * want.n_kept))
        finally:
            owner.close()


def test_whole_file_gunzip_over_the_text(eng, over_the_text):
    """pf_gunzip_device_bgzf of the same file: its loop cuts a decoder call at MAX_TEXT bytes of text"""
    from panfeed_amd import _lib
    u, data, _path, _want = over_the_text
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    _lib.check(eng.L.pf_gunzip_device_bgzf(eng.ctx, data, len(data), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        assert taken.value, eng.L.pf_last_error().decode()
        size, period = bs.M["BGZF_MAX_TEXT"], u.A + u.B
        assert n.value == (2 * bs.PERIODS + 1) * size
        assert C.string_at(out.value, size) == u.C
        bad = [k for k in range(bs.PERIODS) if C.string_at(out.value + size + 2 * size * k, 2 * size) != period]
        assert not bad, bad[:5]
    finally:
        eng.L.pf_free_text(out)
