"""The two text scanners of csrc/pf_rowfilter.hip on the device against the pure-Python models of tests/text_tables.py:
rowfilter_kernel behind RowFilter (bytes for bytes, first-field and last-field mode) and pg_scan_kernel with its table
kernels behind GridBuilder (names, p-value texts, min / max / rows, line and record counts, every cell of every grid).

What the cases are made for: the place of a line end in its 16-byte vector and 32-bit word and the byte that stands next
to it, blocks of 16 bytes to 33 MiB, the 4 095 / 4 096-byte field limits, a scan with more candidates than room, tables
and name arenas that grow while records exist, field forms, and significance keys of every kind of double."""
import itertools
import math

import numpy as np
import pytest

import text_tables as tt
from device_gz_files import member_sizes, write_device_gz

pytestmark = pytest.mark.gpu

HEADER = b"first\tmiddle\tlast\n"
MODES = [True, False]
MODE_IDS = ["first-field", "last-field"]


# ------------------------------------------------------------------------------------------------ row filter
def _scan(text, keys, first_field):
    from panfeed_amd.downstream import RowFilter
    f = RowFilter(keys, first_field=first_field)
    try:
        return f.scan_block(text)
    finally:
        f.close()


def _filter_file(tmp_path, text, keys, first_field, block_bytes):
    from panfeed_amd.downstream import RowFilter
    p = tmp_path / "table.tsv"
    p.write_bytes(HEADER + text)
    f = RowFilter(keys, first_field=first_field)
    try:
        return f.filter_file(str(p), block_bytes)
    finally:
        f.close()


def _same_lines(got, exp):
    """bytes for bytes; a difference is reported by the cases (middle fields) of the lines that differ"""
    if got != exp:
        g, e = got.split(b"\n"), exp.split(b"\n")
        extra = sorted({tt.sweep_case(x) for x in set(g) - set(e)})
        lost = sorted({tt.sweep_case(x) for x in set(e) - set(g)})
        raise AssertionError(f"lines that are not lines of the model: {extra}; lines of the model that are missing: {lost}; "
                             f"{len(g) - 1} lines for {len(e) - 1}")


@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_rowfilter_alignment_sweep(tmp_path, first_field):
    text = tt.rowfilter_alignment_text()
    for keys in (list(tt.RF_KEYS), list(tt.RF_KEYS) + [b""]):
        exp = tt.filter_rows(text, keys, first_field)
        assert exp.count(b"\n") > 60
        got, used = _scan(text, keys, first_field)
        assert used == len(text)
        _same_lines(got, exp)
        for block in tt.BLOCK_SIZES:
            header, rows = _filter_file(tmp_path, text, keys, first_field, block)
            assert header == HEADER
            _same_lines(rows, exp)


@pytest.mark.parametrize("with_empty_key", [False, True], ids=["key", "key-and-empty"])
@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_rowfilter_byte_sweep(first_field, with_empty_key):
    """every byte value next to a line end at each of the four places of the line end in its word.  A 0x0B above a
    newline in one word was once taken for a second line end: the line  0x0B KEY ...  then matched KEY as its first
    field, and with "" among the keys of a last-field filter the "line" 0x0B came back."""
    text = tt.rowfilter_byte_sweep_text()
    keys = [tt.SWEEP_KEY] + ([b""] if with_empty_key else [])
    exp = tt.filter_rows(text, keys, first_field)
    assert exp.count(b"\n") == (0 if first_field else 4 * 254 + 8)
    got, used = _scan(text, keys, first_field)
    assert used == len(text)
    _same_lines(got, exp)


def _field_limit_case():
    """(keys, text): fields and keys of 4 094, 4 095 and 4 096 bytes; lines of 100 000 bytes with short key fields"""
    sizes = (4094, 4095, 4096)
    keys = [b"k" * n for n in sizes] + [b"ab"]
    lines = []
    for n in sizes:
        lines += [b"k" * n + b"\tx\tother", b"other\tx\t" + b"k" * n, b"k" * n, b"k" * (n - 1) + b"j\tx\t" + b"k" * (n - 1) + b"j"]
    lines += [b"ab\t" + b"w" * 100_000 + b"\tab", b"zz\t" + b"w" * 100_000 + b"\tzz", b"w" * 100_000]
    return keys, b"".join(ln + b"\n" for ln in lines)


@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_rowfilter_field_limits(first_field):
    """fields and keys of 4 094 and 4 095 bytes match, of 4 096 bytes never; a line of 100 000 bytes with a short key field"""
    keys, text = _field_limit_case()
    exp = tt.filter_rows(text, keys, first_field)
    assert exp.count(b"\n") == 5 and (b"k" * 4096) not in exp
    got, used = _scan(text, keys, first_field)
    assert used == len(text) and got == exp


def test_rowfilter_more_candidates_than_room():
    """2^20 + 5 matching lines in one block: more than the scan's first guess of the room holds, so it runs a second time
    with what the first asked for.  Every matching line once and in order -- the lines are all alike, so the first scan
    is held by the positions pf_rowfilter_scan itself gives --; the same filter again; a small block after"""
    import ctypes as C

    from panfeed_amd import _lib
    from panfeed_amd.downstream import RowFilter
    n = 2 ** 20 + 5
    text = b"a\n" * n + b"b\nab\t1\n\tq\n"
    f = RowFilter([b"a"], first_field=True)
    try:
        b, e = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        cnt, used = C.c_uint64(), C.c_uint64()
        _lib.check(f.L.pf_rowfilter_scan(f.h, text, len(text), C.byref(b), C.byref(e), C.byref(cnt), C.byref(used)))
        assert (cnt.value, used.value) == (n, len(text))
        begin = np.ctypeslib.as_array(b, (n,))
        assert np.array_equal(begin, 2 * np.arange(n, dtype=np.uint64))
        assert np.array_equal(np.ctypeslib.as_array(e, (n,)), begin + np.uint64(2))
        got, used = f.scan_block(text)
        assert used == len(text) and len(got) == 2 * n and got == b"a\n" * n
        small = b"a\tx\nb\ta\na\nab\n"
        assert f.scan_block(small) == (tt.filter_rows(small, [b"a"], True), len(small))
    finally:
        f.close()


def _large_text(n_target):
    """about n_target bytes of 64-byte lines no key selects, behind a first line of 37 bytes so that no multiple of 64 is
    a line start; lines a key selects at byte 0, at the end and, as 64 lines  ab\\n , over every byte at which a copy of
    the block in 2 or in 8 pieces has a seam"""
    first = b"ab\t" + b"m" * 30 + b"\tab\n"
    buf = bytearray(first + (b"n" * 60 + b"\tnn\n") * ((n_target - len(first)) // 64 + 1))
    n = len(buf)
    buf[n - 64:n] = b"ab\t" + b"m" * 57 + b"\tab\n"
    seams, regions = [], []
    for nt in (2, 8):
        step = -(-n // nt)
        for t in range(1, nt):
            seam = t * step
            seams.append(seam)
            if any(a <= seam < a + 192 for a in regions):            # (half the block, as 1 of 2 and as 4 of 8 pieces)
                continue
            at = len(first) + ((seam - len(first)) // 64 - 1) * 64
            assert len(first) <= at and at + 192 <= n - 64 and at + 64 <= seam < at + 128
            assert all(abs(at - a) >= 192 for a in regions)
            buf[at:at + 192] = b"ab\n" * 64
            regions.append(at)
    return bytes(buf), seams


@pytest.mark.parametrize("mib,pieces", [(9, 2), (33, 8)])
def test_rowfilter_large_blocks(mib, pieces):
    """one block of 8 MiB or more is copied to pinned memory by 2 threads, of 32 MiB or more by 8"""
    text, seams = _large_text(mib << 20)
    assert min(8, len(text) >> 22) == pieces and len(text) % 64 == 37
    assert {text[s:s + 1] for s in seams} <= {b"a", b"b", b"\n"}
    for first_field in MODES:
        exp = tt.filter_rows(text, [b"ab"], first_field)
        assert exp.count(b"\n") == 2 + 64 * 7 and len(seams) == 8
        got, used = _scan(text, [b"ab"], first_field)
        assert used == len(text) and got == exp


@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_rowfilter_key_sets(first_field):
    """no key, one key, the same key several times, a key that holds a tab (it is no field of any line)"""
    text = b"ab\t1\tab\nab\t1\nab\t1\tcd\ncd\t\tab\n1\tab\n\nab\n"
    for keys in ([], [b"ab"], [b"ab", b"ab", b"cd", b"ab"], [b"ab\t1"], [b"ab\t1", b"1\tab", b"cd"], [b"\t"]):
        exp = tt.filter_rows(text, keys, first_field)
        assert _scan(text, keys, first_field) == (exp, len(text)), keys
    assert tt.filter_rows(text, [b"ab\t1", b"\t"], first_field) == b""


# ------------------------------------------------------------------------------------------------ row filter, member route
# The same models through pf_rowfilter_scan_members: the text device-gzipped behind the header line's member, as
# --gpu-compress writes it, inflated on the GPU and scanned where the inflate left it.
@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def _chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def _member_file(eng, tmp_path, text, name="table.tsv.gz"):
    """(path, member sizes) of HEADER + text, device-gzipped"""
    p = tmp_path / name
    write_device_gz(eng, p, HEADER, text)
    return str(p), member_sizes(p.read_bytes())


def _filter_members(path, sizes, keys, first_field, whole_members_per_call=None, times=1):
    """filter_file by the device gunzip route alone, `times` times on one filter: every member inflated on the device"""
    from panfeed_amd.downstream import RowFilter
    block = None if whole_members_per_call is None else whole_members_per_call * max(sizes) + 1
    f = RowFilter(keys, first_field=first_field)
    try:
        got = [f.filter_file(path, block_bytes=block, device_gunzip=True) for _ in range(times)]
        st = f.stats()
    finally:
        f.close()
    assert st["members_inflated"] == times * len(sizes) and st["gunzip_fallbacks"] == 0
    return got[0] if times == 1 else got


def _on_both_blockings(path, sizes, keys, first_field, exp):
    """the default block (the whole file in one call) and one whole member a call (lines carried on the device)"""
    for per_call in (None, 1):
        header, rows = _filter_members(path, sizes, keys, first_field, per_call)
        assert header == HEADER
        _same_lines(rows, exp)


def _model_text(which):
    if which == "byte-sweep":
        return tt.rowfilter_byte_sweep_text(), [[tt.SWEEP_KEY], [tt.SWEEP_KEY, b""]]
    text, C_ = tt.rowfilter_alignment_text(), _chunk_bytes()
    text *= -(-(2 * C_ + 1) // len(text))                       # three members of text at least
    return text, [list(tt.RF_KEYS), list(tt.RF_KEYS) + [b""]]


@pytest.mark.parametrize("which", ["alignment", "byte-sweep"])
def test_member_route_on_the_model_texts(eng, tmp_path, which):
    text, key_lists = _model_text(which)
    path, sizes = _member_file(eng, tmp_path, text)
    C_ = _chunk_bytes()
    assert len(sizes) == 1 + -(-len(text) // C_)
    if which == "alignment":
        # a line lies across a seam between two members: it is carried from one call to the next
        assert len(sizes) >= 1 + 3 and any(text[k * C_ - 1:k * C_] != b"\n" for k in range(1, len(sizes) - 1))
    for first_field in MODES:
        for keys in key_lists:
            exp = tt.filter_rows(text, keys, first_field)
            if which == "alignment":
                assert exp.count(b"\n") > 60
            else:
                assert exp.count(b"\n") == (0 if first_field else 4 * 254 + 8)
            _on_both_blockings(path, sizes, keys, first_field, exp)


@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_member_route_header_only(eng, tmp_path, first_field):
    path, sizes = _member_file(eng, tmp_path, b"")
    assert len(sizes) == 1
    assert _filter_members(path, sizes, list(tt.RF_KEYS) + [b""], first_field) == (HEADER, b"")


@pytest.mark.parametrize("first_field", MODES, ids=MODE_IDS)
def test_member_route_field_limits(eng, tmp_path, first_field):
    """the lines of test_rowfilter_field_limits: those of 100 000 bytes lie across several members, so the carried line
    and the walk to a candidate's line start cross member seams"""
    keys, text = _field_limit_case()
    path, sizes = _member_file(eng, tmp_path, text)
    assert len(sizes) > 1 + 3 * 100_000 // _chunk_bytes()
    exp = tt.filter_rows(text, keys, first_field)
    assert exp.count(b"\n") == 5 and (b"k" * 4096) not in exp
    _on_both_blockings(path, sizes, keys, first_field, exp)


def test_member_route_more_candidates_than_room(eng, tmp_path):
    """2^20 + 5 matching lines in one call, about 2 MiB of text in 64 members: the scan runs a second time with the room
    the first asked for, and every candidate's line is gathered; the same filter again"""
    n = 2 ** 20 + 5
    text = b"a\n" * n + b"b\nab\t1\n\tq\n"
    path, sizes = _member_file(eng, tmp_path, text)
    assert len(sizes) == 1 + -(-len(text) // _chunk_bytes())
    for header, rows in _filter_members(path, sizes, [b"a"], True, times=2):
        assert header == HEADER and len(rows) == 2 * n and rows == b"a\n" * n


def test_member_route_unfinished_member_over_a_slot_is_refused_at_once():
    """a block, not the file's last, that holds no whole member: short of a slot's bytes and a head it is taken with
    nothing consumed (the caller reads on); from that size on a member this decoder takes would have ended, and the
    block is refused there and then -- not taken, as one whole-file member of gzip's is -- not when the file ends"""
    import inflate_cases as ic

    from panfeed_amd import _lib
    from panfeed_amd.downstream import RowFilter
    limit = ic.slot_bytes(_chunk_bytes()) + len(ic.HEAD)
    data = ic.HEAD + b"\x55" * limit                         # (no second member head in it)
    f = RowFilter([b"a"], first_field=True)
    try:
        _lib.check(f.L.pf_rowfilter_members_begin(f.h, 1))
        assert f.scan_members(data[:limit - 1], False) == (b"", 0, True)
        assert f.scan_members(data[:limit], False) == (b"", 0, False)
        assert b"not taken" in f.L.pf_last_error()
        assert f.scan_members(data, False) == (b"", 0, False)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ plot scan
NAN = float("nan")
SPECIALS = (NAN, -math.inf, -2.5, -0.0, 0.0, 5e-324, 1.5, math.inf)


def _by_number(text):
    """a double for a p-value text, chosen by the test: the digits in the text pick one of SPECIALS"""
    digits = bytes(c for c in text if 48 <= c <= 57)
    return SPECIALS[int(digits or b"0") % len(SPECIALS)]


def _key_of(value):
    from panfeed_amd.plot import _keys
    return 0 if value is None else int(_keys(np.array([value], dtype=np.float64))[0])


def _check(gb, m, sig_of=_by_number):
    """everything a finished GridBuilder gives against the model; clusters by name (slot order is hash order)"""
    names = [c.encode() for c in gb.clusters]
    assert len(set(names)) == len(names) and set(names) == set(m.clusters)
    for i, nm in enumerate(names):
        mn, mx, rows = m.clusters[nm]
        assert int(gb.rows[i]) == rows, nm
        if rows:
            assert (int(gb.min[i]), int(gb.max[i])) == (mn, mx), nm
    texts = gb.pvalue_texts
    assert len(set(texts)) == len(texts) and set(texts) == m.texts
    st = gb.stats()
    assert (st["lines"], st["records"], gb.n_records) == (m.lines, m.records, m.records)
    gb.set_significance(np.array([sig_of(t) for t in texts], dtype=np.float64))
    cells = {}
    for (nm, sid, pos), cell in m.cells.items():
        cells.setdefault(nm, []).append((sid, pos, cell))
    ids = [i for i in range(len(names)) if gb.rows[i]]
    if not ids:
        return
    for i, (key, cnt) in zip(ids, gb.grids(ids)):
        mn = m.clusters[names[i]][0]
        exp_cnt = np.zeros(key.shape, np.uint64)
        exp_key = np.zeros(key.shape, np.uint64)
        exp_letter = np.zeros(key.shape, np.uint64)
        for sid, pos, cell in cells[names[i]]:
            exp_cnt[sid, pos - mn] = cell.count
            exp_key[sid, pos - mn] = _key_of(tt.ieee_max([sig_of(t) for t in cell.texts]))
            exp_letter[sid, pos - mn] = cell.letters[0]
        assert np.array_equal(cnt >> np.uint64(32), exp_cnt), names[i]
        assert np.array_equal(key, exp_key), names[i]
        one = exp_cnt == 1
        assert np.array_equal((cnt & np.uint64(0xFFFFFFFF))[one], exp_letter[one]), names[i]


def _builder(tmp_path, body, strains, columns=tt.PLOT_COLUMNS, start=None, stop=None, block_bytes=None, header=tt.PLOT_HEADER):
    """a GridBuilder that has scanned header + body and is finished"""
    from panfeed_amd.plot import GridBuilder
    p = tmp_path / "annotated.tsv"
    p.write_bytes(header + body)
    gb = GridBuilder([s.decode() for s in strains], columns, start, stop)
    try:
        gb.scan_file(str(p), block_bytes)
        gb.finish()
    except Exception:
        gb.close()
        raise
    return gb


def _run(tmp_path, body, strains, columns=tt.PLOT_COLUMNS, start=None, stop=None, block_bytes=None, sig_of=_by_number,
         header=tt.PLOT_HEADER):
    m = tt.plot_model(tt.as_file(body), columns, strains, start, stop)
    gb = _builder(tmp_path, body, strains, columns, start, stop, block_bytes, header)
    try:
        _check(gb, m, sig_of)
    finally:
        gb.close()
    return m


@pytest.mark.parametrize("block_bytes", [None, 64, 257])
def test_plot_alignment_sweep(tmp_path, block_bytes):
    m = _run(tmp_path, tt.plot_alignment_text(), tt.PLOT_STRAINS, block_bytes=block_bytes)
    assert m.records > 100 and len(m.texts) == 9


@pytest.mark.parametrize("block_bytes", [None, 64, 257])
def test_plot_byte_sweep(tmp_path, block_bytes):
    """every byte of 0x01-0x7F in front of a cluster name, behind a line end at each of the four places in its word.  A
    0x0B there once made a second record, under the name without its first byte, and a second line"""
    m = _run(tmp_path, tt.plot_byte_sweep_text(), tt.PLOT_STRAINS, block_bytes=block_bytes)
    assert len(m.clusters) == 125 + 2 + 1 and tt.PLOT_NAME not in m.clusters and m.lines == m.records == 2 * 4 * 127


def test_plot_significance_keys(tmp_path):
    """every kind of double as a significance, alone in a cell and every two of them together in one: the cell's key is
    that of the IEEE maximum of its non-NaN values, 0 where there is none"""
    rows = []
    for i, (a, b) in enumerate(itertools.product(range(len(SPECIALS)), repeat=2)):
        rows += [b"sig\ts0\t%d\tA\t1\tp%d\n" % (i, a), b"sig\ts0\t%d\tC\t1\tq%d\n" % (i, b)]
    rows += [b"sig\ts1\t%d\tG\t1\tp%d\n" % (i, i) for i in range(len(SPECIALS))]
    m = _run(tmp_path, b"".join(rows), [b"s0", b"s1"])
    assert len(m.texts) == 2 * len(SPECIALS) and {c.count for c in m.cells.values()} == {1, 2}
    assert _key_of(tt.ieee_max([-0.0, 0.0])) == _key_of(0.0) != _key_of(-0.0) and _key_of(NAN) == 0 == _key_of(None)


WIDE_HEADER = b"\t".join(b"col%d" % i for i in range(13)) + b"\n"


@pytest.mark.parametrize("columns", [[0, 9, 2, 11, 7, 12], [5, 0, 12, 3, 8, 1]], ids=["pvalue-last", "cluster-not-first"])
def test_plot_columns(tmp_path, columns):
    """the six fields anywhere in a 13-column table; lines that are too short are counted and not kept, fields behind the
    13th are ignored, blank lines are no lines"""
    lines = []
    for i in range(60):
        f = [b"f%d_%d" % (c, i % 4) for c in range(13)]
        vals = (b"g%d" % (i % 5), tt.PLOT_STRAINS[i % 6], b"%d" % (i % 9 - 3), (b"ACGT", b"gatc", b"")[i % 3],
                (b"-1", b"1")[i % 2], b"p%d" % (i % 7))
        for c, v in zip(columns, vals):
            f[c] = v
        if i % 10 == 3:
            f = f[:max(columns)]                     # the line ends one field early
        elif i % 10 == 4:
            f = f[:12 - i % 7]
        elif i % 10 == 5:
            f += [b"extra", b""]
        lines.append(b"\t".join(f))
        if i % 13 == 6:
            lines.append(b"")
    body = b"".join(ln + b"\n" for ln in lines)
    for block_bytes in (None, 257):
        m = _run(tmp_path, body, tt.PLOT_STRAINS, columns, block_bytes=block_bytes, header=WIDE_HEADER)
        assert m.lines == 60 and 40 <= m.records < 50


def _forms_body():
    rows = []
    for i, pos in enumerate((b"5", b"-3", b"+5", b"007", b"-0", b"2147483647", b"-2147483647", b"", b"abc")):
        rows.append(b"pos%d\ts0\t%s\tACGT\t1\tp%d\n" % (i, pos, i))
    for i, strand in enumerate((b"-1", b"-1.0", b"-01", b"1", b"+1", b"0", b"-11", b"", b"-")):
        for j, kmer in enumerate((b"acgT", b"GGa", b"N", b"c", b"t", b"", b"aN", b"Xg")):
            rows.append(b"strand\ts1\t%d\t%s\t%s\tp%d\n" % (10 * i + j, kmer, strand, j))
    rows += [b"zoom\ts0\t%d\tA\t1\tp1\n" % x for x in range(-6, 7)]
    return b"".join(rows)


@pytest.mark.parametrize("zoom", [(None, None), (-3, 5), (5, 5), (6, 4), (-6, -4), (-2147483647, 2147483647)],
                         ids=["all", "-3..5", "5..5", "6..4", "-6..-4", "widest"])
def test_plot_field_forms(tmp_path, zoom):
    """gene_start as 5, -3, +5, 007, -0 and at both ends of 32 bits; an empty or non-numeric gene_start drops the row and
    keeps the cluster listed; the strand forms that are and are not -1; k-mers in lower case, with N, of one letter and
    empty; the zoom's ends are inclusive, a window with start > stop keeps nothing"""
    m = _run(tmp_path, _forms_body(), [b"s0", b"s1"], start=zoom[0], stop=zoom[1])
    assert m.clusters[b"pos7"] == m.clusters[b"pos8"] == (None, None, 0)
    if zoom[0] is None or zoom[0] < -100:
        assert m.clusters[b"pos5"] == (2147483647, 2147483647, 1) and m.clusters[b"pos6"] == (-2147483647, -2147483647, 1)
        assert m.clusters[b"pos3"] == (7, 7, 1) and m.clusters[b"pos4"] == (0, 0, 1) and m.clusters[b"zoom"] == (-6, 6, 13)
    if zoom == (6, 4):
        assert m.records == 0 and len(m.clusters) == 11
    if zoom == (5, 5):
        assert m.clusters[b"zoom"] == (5, 5, 1) and m.clusters[b"pos0"][2] == m.clusters[b"pos2"][2] == 1


@pytest.mark.parametrize("pos", [b"2147483648", b"-2147483648"])
def test_plot_gene_start_outside_32_bits_is_refused(tmp_path, pos):
    from panfeed_amd import _lib
    body = b"g\ts0\t1\tA\t1\tp\n" + b"g\ts0\t" + pos + b"\tA\t1\tp\n"
    with pytest.raises(tt.ModelArgumentError):
        tt.plot_model(body, tt.PLOT_COLUMNS, [b"s0"])
    with pytest.raises(_lib.PanfeedHipError) as ei:
        _builder(tmp_path, body, [b"s0"]).close()
    assert ei.value.status == _lib.ERR_ARG
    _run(tmp_path, b"g\ts0\t1\tA\t1\tp\n", [b"s0"])               # a fresh builder works


@pytest.mark.parametrize("with_empty_name", [False, True])
def test_plot_strain_names(tmp_path, with_empty_name):
    """a name twice in the phenotype list (its first id counts), names that are prefixes of one another, names equal but
    for their last byte, the empty strain field -- with and without an empty name in the list"""
    strains = [b"s1", b"s1x", b"s1", b"s", b"ab_1", b"ab_2"] + ([b""] if with_empty_name else [])
    fields = [b"s1", b"s1x", b"s", b"ab_1", b"ab_2", b"", b"s1xy", b"ab_", b"ab_3", b"S1", b"1", b"s1\r"]
    body = b"".join(b"g%d\t%s\t%d\tA\t1\tp%d\n" % (i % 3, f, i % 4, i % 5) for i, f in enumerate(fields * 3))
    m = _run(tmp_path, body, strains)
    assert {sid for (_c, sid, _p) in m.cells} == {0, 1, 3, 4, 5} | ({6} if with_empty_name else set())
    assert m.records == 3 * (6 if with_empty_name else 5) and m.lines == 36


def test_plot_tables_grow_with_records_present(tmp_path):
    """5 000 rows, each with a cluster name and a p-value text of its own, in blocks of 1 024 bytes: both tables start at
    1 024 slots and are moved to 2 048, 4 096, 8 192 and 16 384 while records point into them"""
    body = b"".join(b"c%05d\ts%d\t%d\t%s\t1\tq%05d\n" % (i, i % 4, i % 7 - 3, (b"ACGT", b"gT", b"")[i % 3], (i * 7919) % 5000)
                    for i in range(5000))
    m = _run(tmp_path, body, [b"s0", b"s1", b"s2", b"s3"], block_bytes=1024)
    assert len(m.clusters) == len(m.texts) == m.records == 5000


def _long_name(i, n=3600):
    """n bytes of printable ASCII that differ from name to name at the front and all along"""
    return b"n%04d_" % i + ((np.arange(n - 6, dtype=np.int64) * (2 * i + 1) + i * i) % 94 + 33).astype(np.uint8).tobytes()


def test_plot_name_arena_grows(tmp_path):
    """320 cluster names of 3 600 bytes each in blocks of 8 192 bytes: over 1 MiB of names behind a first arena of 1 MiB,
    which is copied to a larger one; every name comes back whole.  A name of 4 095 bytes is the longest that passes"""
    names = [_long_name(i) for i in range(320)] + [_long_name(999, 4095)]
    assert len(set(names)) == 321 and sum(len(x) for x in names[:320]) > (1 << 20)
    body = b"".join(b"%s\ts%d\t%d\tA\t1\tp%d\n" % (nm, i % 2, i, i % 11) for i, nm in enumerate(names))
    m = _run(tmp_path, body, [b"s0", b"s1"], block_bytes=8192)
    assert m.records == 321 and max(len(x) for x in m.clusters) == 4095


@pytest.mark.parametrize("which", ["cluster", "pvalue"])
def test_plot_field_of_4096_bytes_is_refused(tmp_path, which):
    from panfeed_amd import _lib
    long = _long_name(5, 4096)
    row = (long + b"\ts0\t2\tA\t1\tp1\n") if which == "cluster" else (b"g\ts0\t2\tA\t1\t" + long + b"\n")
    body = b"g\ts0\t1\tA\t1\tp0\n" + row
    with pytest.raises(tt.ModelArgumentError):
        tt.plot_model(body, tt.PLOT_COLUMNS, [b"s0"])
    with pytest.raises(_lib.PanfeedHipError) as ei:
        _builder(tmp_path, body, [b"s0"]).close()
    assert ei.value.status == _lib.ERR_ARG
    # one byte less passes, in a fresh builder
    _run(tmp_path, b"g\ts0\t1\tA\t1\tp0\n" + row.replace(long, long[:4095]), [b"s0"])
