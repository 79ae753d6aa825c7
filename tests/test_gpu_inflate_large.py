"""The large-member gunzip route on the GPU (gz_find_kernel, gz_marker_kernel, gz_chain_kernel, gz_bytes_kernel,
csrc/pf_deflate.hip): the files of tests/inflate_large_cases.py through the whole-buffer call against zlib's text and the
host model's piece counts, and through the device text feed's four owners -- a member that spans calls, refusals with
their fall-back to the host, the switch off, the tools' flag."""
import ctypes as C
import gzip
import io
import json
import os
import sys

import pytest

from conftest import GOLDEN, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
import inflate_large_cases as lc  # noqa: E402
import join_tables as jt  # noqa: E402
import test_gpu_plot_members as pm  # noqa: E402
import test_inflate_large_host as th  # noqa: E402
import text_tables as tt  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN_BLOCKS = (4096, 1000003, None)         # pass_member_file's reads: a member over many calls, and the one-block pass
PIECE = 200


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def device_large(eng, data, piece_bytes):
    """(text or None when not taken, [found, live, dropped, members], the library's message)"""
    from panfeed_amd import _lib
    out, n, taken, pieces = C.c_void_p(), C.c_uint64(), C.c_int(), (C.c_uint64 * 4)()
    _lib.check(eng.L.pf_gunzip_device_large(eng.ctx, data, len(data), piece_bytes, C.byref(out), C.byref(n), C.byref(taken), pieces))
    try:
        if not taken.value:
            return None, list(pieces), eng.L.pf_last_error().decode()
        return (C.string_at(out, n.value) if n.value else b""), list(pieces), ""
    finally:
        eng.L.pf_free_text(out)


def many_blocks_gz(text):
    """one gzip member of many small deflate blocks (zlib at memLevel 1) under a head with a file name, as gzip.open writes"""
    return lc.member(lc.deflate(text, 6, 1), text, lc.FNAME, mtime=1700000000)


# ---- the whole-buffer call
@pytest.mark.parametrize("name", [c.name for c in th.accepted()])
def test_accepted_files_give_zlib_s_text_and_the_host_model_s_pieces(eng, name):
    c = next(c for c in th.accepted() if c.name == name)
    for p in c.pieces:
        got, pieces, why = device_large(eng, c.data, p)
        want = th.host_results()[name, p]
        assert got == c.text, (p, why or "another text")
        assert pieces == want[1], p                      # found, live and dropped pieces, members: the host model's
    ms = C.c_float()
    assert eng.L.pf_gunzip_device_last_ms(eng.ctx, C.byref(ms)) == 0 and ms.value > 0


def test_false_starts_are_dropped(eng):
    c = next(c for c in th.accepted() if c.name == "stored_stream_inside")
    got, (found, live, dropped, members), _ = device_large(eng, c.data, 64)
    assert got == c.text and dropped > 0 and found == live + dropped and members == 1


def test_refused_files_are_not_taken(eng):
    for r in th.refused():
        for p in r.pieces:
            got, _, why = device_large(eng, r.data, p)
            host = th.host_large(r.data, p)
            assert got is None and why.rsplit(": ", 1)[1] == host[2].rsplit(": ", 1)[1], (r.name, p, why)
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    assert eng.L.pf_gunzip_device_large(eng.ctx, b"x", 1, 63, C.byref(out), C.byref(n), C.byref(taken), None) != 0


# ---- through the feed: each owner's answer over a file, as a comparable value
def _rowfilter(path, **kw):
    from panfeed_amd.downstream import RowFilter
    f = RowFilter(list(tt.RF_KEYS), first_field=True)
    try:
        got = f.filter_file(str(path), **kw)
        return got, f.stats(), f.large_stats()
    finally:
        f.close()


JOIN_KEYS = [(b"g", b"ACG"), (b"full", b"CCA")]


def _kmerjoin(path, **kw):
    from panfeed_amd.downstream import KJ_RAW, KmerJoin
    kj = KmerJoin([(b"g", 0), (b"full", 1)], 2, JOIN_KEYS, [b"t0", b"u0"], [b"t1.0", b"u1.0"], b"")
    try:
        plan = kj.survey_file(str(path), **kw)
        texts = {}
        for bunch in (0, 1):
            for mode in (0, KJ_RAW):
                out = []
                kj.join_file(str(path), bunch, mode, lambda piece: out.append(bytes(piece)), block_bytes=kw.get("block_bytes"))
                texts[bunch, mode] = b"".join(out)
        return (plan, texts), kj.stats(), kj.large_stats()
    finally:
        kj.close()


def _assocfilter(path, **kw):
    from panfeed_amd.downstream import AssocFilter
    f = AssocFilter(at.PVALUE_FIELD, 8, 1e-8)
    try:
        kept = f.filter_file(str(path), **kw)
        cols = f.columns()
        return (kept, cols), f.stats(), f.large_stats()
    finally:
        f.close()


def _plotgrid(path, **kw):
    from panfeed_amd.plot import GridBuilder
    gb = GridBuilder([s.decode() for s in tt.PLOT_STRAINS], tt.PLOT_COLUMNS)
    try:
        gb.scan_file(str(path), kw.pop("block_bytes", None), kw.pop("device_gunzip", None), **kw)
        gb.finish()
        return pm._snapshot(gb), gb.stats(), gb.large_stats()
    finally:
        gb.close()


def _kmers_table():
    return jt.handmade(rows_per_cluster=300, final_newline=True)["kmers"]


def _filler(n, fields):
    """n rows no key matches, of text that does not compress away: the small tables between them make a member of many blocks"""
    import random
    rng = random.Random(n)
    return [fields(i, "".join(rng.choice("ACGT") for _ in range(31)).encode()) for i in range(n)]


def _rowfilter_table():
    rows = tt.rowfilter_alignment_text().splitlines(keepends=True)
    fill = _filler(900, lambda i, kmer: b"row%d\t%s\n" % (i, kmer))
    return b"key\tvalue\n" + b"".join(r + b"".join(fill[9 * i:9 * i + 9]) for i, r in enumerate(rows)) + b"".join(fill[9 * len(rows):])


def _plot_table():
    rows = tt.plot_alignment_text().splitlines(keepends=True)
    fill = _filler(900, lambda i, kmer: b"c%d\t%s\t%d\t%s\t%s\tp%d\n" % (i % 7, tt.PLOT_STRAINS[i % 6], i % 13 - 5, kmer, (b"1", b"-1")[i % 2], i % 5))
    return tt.PLOT_HEADER + b"".join(r + b"".join(fill[9 * i:9 * i + 9]) for i, r in enumerate(rows)) + b"".join(fill[9 * len(rows):])


OWNERS = {"rowfilter": (_rowfilter, _rowfilter_table), "kmerjoin": (_kmerjoin, _kmers_table),
          "assocfilter": (_assocfilter, lambda: at.seeded_table(5)), "plotgrid": (_plotgrid, _plot_table)}


@pytest.fixture(scope="module")
def owner_files(tmp_path_factory):
    """per owner: its table, the plain file, the one-member .gz of many blocks, and the plain file's answer -- made once"""
    d = tmp_path_factory.mktemp("large_members")
    out = {}
    for name, (run, make) in OWNERS.items():
        text = make()
        plain, gz = d / f"{name}.tsv", d / f"{name}.tsv.gz"
        plain.write_bytes(text)
        gz.write_bytes(many_blocks_gz(text))
        assert len(gz.read_bytes()) > 2 * 4096                   # the member spans several reads of 4 096 bytes
        out[name] = (text, plain, gz, run(plain)[0])
    return out


@pytest.mark.parametrize("block_bytes", SPAN_BLOCKS, ids=["reads_of_4096", "reads_of_1000003", "default_read"])
@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_a_member_that_spans_calls_gives_the_plain_file_s_answer(owner_files, owner, block_bytes):
    """the same rows, the same counters and the same text bytes whatever the reads: a call takes the pieces it can confirm,
    the next one goes on from the byte that holds the next block"""
    run = OWNERS[owner][0]
    text, plain, gz, want = owner_files[owner]
    got, st, large = run(gz, block_bytes=block_bytes, device_gunzip=True, large_members=True, piece_bytes=PIECE)
    assert got == want
    passes = 5 if owner == "kmerjoin" else 1                     # (the survey and four joins read the file)
    assert st["text_bytes_inflated"] == passes * len(text) and st["members_inflated"] == passes
    assert large["large_members"] == passes and large["pieces_live"] >= 10 * passes and large["pieces_dropped"] == 0
    assert large["find_ms"] > 0 and large["marker_ms"] > 0 and large["chain_ms"] > 0 and large["bytes_ms"] > 0


def test_the_default_piece_and_a_gzip_compress_file(owner_files, tmp_path):
    text, plain, _, want = owner_files["rowfilter"]
    p = tmp_path / "whole.tsv.gz"
    p.write_bytes(gzip.compress(text))
    for kw in ({"device_gunzip": True}, {}):
        got, st, large = _rowfilter(p, large_members=True, **kw)
        assert got == want and st["gunzip_fallbacks"] == 0 and st["text_bytes_inflated"] == len(text) and large["large_members"] == 1


def test_both_routes_in_one_file(eng, tmp_path):
    """a large member between small --gpu-compress members: the small ones by the kernels that always took them, the large
    one by the new route, no fallback"""
    c = next(c for c in th.accepted() if c.name == "large_between_small")
    rows = c.text.split(b"\n")
    keys = sorted({r.split(b"\t")[0] for r in rows[1:] if r})[:5]
    plain, gz = tmp_path / "mixed.tsv", tmp_path / "mixed.tsv.gz"
    plain.write_bytes(c.text)
    gz.write_bytes(c.data)
    from panfeed_amd.downstream import RowFilter
    f = RowFilter(keys, first_field=True)
    try:
        want = f.filter_file(str(plain))
        assert want[1]
        for block in (4096, None):
            before = f.stats()["members_inflated"], f.large_stats()["large_members"]
            assert f.filter_file(str(gz), block_bytes=block, large_members=True, piece_bytes=PIECE) == want
            st, large = f.stats(), f.large_stats()
            assert large["large_members"] - before[1] == 1 and st["members_inflated"] - before[0] >= 4 and st["gunzip_fallbacks"] == 0
    finally:
        f.close()


def test_large_members_in_a_row_are_taken_side_by_side(tmp_path):
    """four large members under one signature, in reads of 4 096 bytes and in one: the members behind the first are found
    from it, also when it was open as its call began, so a call takes more than one member's pieces"""
    from panfeed_amd.downstream import RowFilter
    c = next(c for c in th.accepted() if c.name == "large_members_in_a_row")
    keys = sorted({r.split(b"\t")[0] for r in c.text.split(b"\n")[1:] if r})[:5]
    plain, gz = tmp_path / "row.tsv", tmp_path / "row.tsv.gz"
    plain.write_bytes(c.text)
    gz.write_bytes(c.data)
    for block in (4096, None):
        f = RowFilter(keys, first_field=True)
        try:
            want = f.filter_file(str(plain))
            assert want[1] and f.filter_file(str(gz), block_bytes=block, large_members=True, piece_bytes=PIECE) == want
            st, large = f.stats(), f.large_stats()
            assert large["large_members"] == 4 and large["pieces_dropped"] == 0 and st["gunzip_fallbacks"] == 0
            assert st["text_bytes_inflated"] == len(c.text)
        finally:
            f.close()


# ---- refusals: not taken, then the host's rows or the host's exception, nothing half-scanned left in the owner
@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_a_refused_file_falls_back_to_the_host(owner_files, owner, tmp_path):
    from panfeed_amd.downstream import NotTaken
    run = OWNERS[owner][0]
    text, plain, gz, want = owner_files[owner]
    raw = gz.read_bytes()
    off_by_one = tmp_path / "isize.tsv.gz"
    off_by_one.write_bytes(raw[:-4] + ((len(text) + 1) & 0xFFFFFFFF).to_bytes(4, "little"))
    reserved = tmp_path / "reserved.tsv.gz"
    reserved.write_bytes(raw[:3] + bytes([raw[3] | 0x20]) + raw[4:])
    with pytest.raises(NotTaken):
        run(reserved, device_gunzip=True, large_members=True, piece_bytes=PIECE)
    got, st, large = run(reserved, large_members=True, piece_bytes=PIECE, block_bytes=4096)      # (gzip does not look at the bit)
    assert got == want and large["large_members"] == 0
    for block in (4096, None):
        with pytest.raises(Exception) as host:
            run(off_by_one, device_gunzip=False)
        with pytest.raises(Exception) as auto:
            run(off_by_one, large_members=True, piece_bytes=PIECE, block_bytes=block)
        assert type(auto.value) is type(host.value) and not isinstance(host.value, (AssertionError, NotTaken))


@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_damaged_files_raise_what_gzip_raises(owner_files, owner, tmp_path):
    """a flipped bit, a cut in the last block and in the tail, a first-piece match before the member's start, through every
    owner in reads of 4 096 bytes: calls before the damage have scanned rows, then the block is not taken, the owner starts
    over and the host's exception comes out; after it the same owner gives the plain file's answer"""
    from panfeed_amd.downstream import NotTaken
    run = OWNERS[owner][0]
    text, plain, gz, want = owner_files[owner]
    raw = gz.read_bytes()
    flipped = bytearray(raw)
    flipped[len(raw) // 2] ^= 0x10
    first = lc.ie.write([lc.ie.dynamic(list(text[:text.index(b"\n") + 1]) + [("far", 5, 400)] + list(b"\n"), lc.ie.FULL_LL, lc.ie.FULL_D, True)])
    damaged = {"flipped": bytes(flipped), "cut_in_last_block": raw[:-8 - 5], "cut_in_tail": raw[:-3],
               "match_before_start": lc.member(first.body, b"")}
    for name, data in damaged.items():
        p = tmp_path / f"{name}.tsv.gz"
        p.write_bytes(data)
        with pytest.raises(Exception) as host:
            run(p, device_gunzip=False)
        with pytest.raises(Exception) as auto:
            run(p, large_members=True, piece_bytes=PIECE, block_bytes=4096)
        assert type(auto.value) is type(host.value) and not isinstance(host.value, (AssertionError, NotTaken)), name
        with pytest.raises(NotTaken):
            run(p, device_gunzip=True, large_members=True, piece_bytes=PIECE)


def test_an_owner_is_whole_after_a_refusal_in_mid_file(owner_files, tmp_path):
    """one owner, three files in a row: a file cut in its tail is refused at its last call, after every row was scanned on the
    device -- the automatic route starts over and the host raises; the good file behind it gives exactly the plain file's rows
    (nothing of the refused pass is left in the owner), by the route, with no further fallback"""
    from panfeed_amd.downstream import RowFilter
    text, plain, gz, want = owner_files["rowfilter"]
    cut = tmp_path / "cut.tsv.gz"
    cut.write_bytes(gz.read_bytes()[:-3])
    f = RowFilter(list(tt.RF_KEYS), first_field=True)
    try:
        f.set_large_members(True, PIECE)
        with pytest.raises(EOFError):
            f.filter_file(str(cut), block_bytes=4096)
        assert f.stats()["gunzip_fallbacks"] == 1 and f.large_stats()["large_members"] == 0
        assert f.filter_file(str(gz), block_bytes=4096) == want
        assert f.stats()["gunzip_fallbacks"] == 1 and f.large_stats()["large_members"] == 1
    finally:
        f.close()


@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_the_owner_s_switch_holds_for_file_calls_that_do_not_name_it(owner_files, owner):
    """set_large_members(True, piece) and then a file call without the argument: the route is on, with that piece; the
    argument given as False turns it off again"""
    from panfeed_amd import plot
    from panfeed_amd.downstream import AssocFilter, KmerJoin, NotTaken, RowFilter
    text, plain, gz, want = owner_files[owner]
    o = {"rowfilter": lambda: RowFilter(list(tt.RF_KEYS), first_field=True), "assocfilter": lambda: AssocFilter(at.PVALUE_FIELD, 8, 1e-8),
         "kmerjoin": lambda: KmerJoin([(b"g", 0), (b"full", 1)], 2, JOIN_KEYS, [b"t0", b"u0"], [b"t1.0", b"u1.0"], b""),
         "plotgrid": lambda: plot.GridBuilder([s.decode() for s in tt.PLOT_STRAINS], tt.PLOT_COLUMNS)}[owner]()
    call = {"rowfilter": "filter_file", "assocfilter": "filter_file", "kmerjoin": "survey_file", "plotgrid": "scan_file"}[owner]
    try:
        o.set_large_members(True, PIECE)
        getattr(o, call)(str(gz))
        large = o.large_stats()
        assert large["large_members"] == 1 and large["pieces_live"] >= 10 and o.piece_bytes == PIECE and o.large_members
        with pytest.raises(NotTaken):
            getattr(o, call)(str(gz), device_gunzip=True, large_members=False)
        assert not o.large_members
    finally:
        o.close()


def test_a_header_line_the_feed_cannot_peel_is_not_taken_with_the_switch_on(eng, tmp_path):
    """small members -- the device encoder's, the header line across three of them -- whose first line runs over 64 KiB: the
    small-member route takes them and the feed refuses the block for real -- the switch does not send what
    the header stage refuses to the large route, and no line is scanned in the header's place -- and the host reads the file"""
    from device_gz_files import device_gzip
    from panfeed_amd.downstream import RowFilter
    header = b"key\t" + b"h" * 70000 + b"\n"
    rows = b"".join(b"%s\tv%d\n" % (tt.RF_KEYS[i % 3], i) for i in range(50)) + b"other\tx\n"
    plain, gz = tmp_path / "long_header.tsv", tmp_path / "long_header.tsv.gz"
    plain.write_bytes(header + rows)
    gz.write_bytes(device_gzip(eng, header + rows))
    assert gzip.decompress(gz.read_bytes()) == header + rows
    f = RowFilter(list(tt.RF_KEYS), first_field=True)
    try:
        want = f.filter_file(str(plain))
        assert want[0] == header and want[1].count(b"\n") == 50
        assert f.filter_file(str(gz), large_members=True, piece_bytes=PIECE) == want
        assert f.stats()["gunzip_fallbacks"] == 1 and f.large_stats()["large_members"] == 0
    finally:
        f.close()


# ---- the switch off: today's behaviour
def test_without_the_switch_such_files_go_the_host_way(owner_files, tmp_path):
    from panfeed_amd.downstream import NotTaken
    text, plain, gz, want = owner_files["rowfilter"]
    p = tmp_path / "whole.tsv.gz"
    p.write_bytes(gzip.compress(text))
    with pytest.raises(NotTaken):
        _rowfilter(p, device_gunzip=True)
    got, st, large = _rowfilter(p)
    assert got == want and st["gunzip_fallbacks"] == 1 and st["text_bytes_inflated"] == 0
    assert large["large_members"] == 0 and large["pieces_found"] == 0
    got, st, large = _rowfilter(gz)                              # (a head with a file name is not even tried)
    assert got == want and st["gunzip_fallbacks"] == 0 and st["text_bytes_inflated"] == 0


# ---- the tools
with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}


def test_get_kmers_with_the_flag_prints_the_plain_run_s_bytes(tmp_path):
    from panfeed_amd import downstream
    from panfeed_amd.downstream import AssocFilter, KmerJoin, RowFilter
    fx = FIX[0]
    run = next(r for r in fx["runs"] if r["tool"] == "get_kmers" and r["stdout"])
    exp = CASES[fx["case"]]["expect"]
    files = {"kmers.tsv": exp["kmers.tsv"].encode(), "kmers_to_hashes.tsv": exp["kmers_to_hashes.tsv"].encode(), "assoc.tsv": fx["associations"].encode()}
    for name, text in files.items():
        (tmp_path / name).write_bytes(text)
        (tmp_path / (name + ".gz")).write_bytes(gzip.compress(text))

    def go(suffix, extra):
        out = io.StringIO()
        argv = ["-a", str(tmp_path / ("assoc.tsv" + suffix)), "-p", str(tmp_path / ("kmers_to_hashes.tsv" + suffix)),
                "-k", str(tmp_path / ("kmers.tsv" + suffix))] + run["args"] + extra
        assert downstream.get_kmers(argv, out=out) in (None, run["rc"])
        return out.getvalue()

    def counts():
        return tuple(cls.device_gunzip_files for cls in (AssocFilter, RowFilter, KmerJoin)), tuple(cls.fallback_files for cls in (AssocFilter, RowFilter, KmerJoin))

    plain = go("", [])
    assert plain
    before = counts()
    assert go(".gz", ["--gpu-gunzip-large"]) == plain
    after = counts()
    assert all(b > a for a, b in zip(before[0], after[0])) and after[1] == before[1]         # all three inputs on the device, no fallback
    assert go(".gz", ["--gpu-gunzip-large", "--host-gunzip"]) == plain
    assert counts() == after                                                             # nothing inflated on the device
