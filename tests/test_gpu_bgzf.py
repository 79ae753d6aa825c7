"""BGZF on the device: pf_gunzip_device_bgzf (gz_inflate64_kernel for the members of more than a chunk of text, the plain
kernel for the others) over the files of tests/bgzf_cases.py, the encoder's framing under PF_GZ_BGZF, the four owners of
the device text feed over maker-written BGZF copies of their small tables, and `panfeed --gpu-compress --bgzf` end to end.
Expected text never comes from the device route: zlib, the host route and the host model give it."""
import ctypes as C
import gzip
import io
import json
import os
import struct
import sys
import zlib

import pytest

from conftest import REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_tables as at  # noqa: E402
import bgzf_cases as bc  # noqa: E402
import deflate_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


def _text(L, call):
    from panfeed_amd import _lib
    out, n = C.c_void_p(), C.c_uint64()
    _lib.check(call(C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value) if n.value else b""
    finally:
        L.pf_free_text(out)


def _gunzip(L, call):
    """(text or None when not taken, the library's message)"""
    taken = C.c_int()
    text = _text(L, lambda out, n: call(out, n, C.byref(taken)))
    return (text, "") if taken.value else (None, L.pf_last_error().decode())


def device_gunzip(eng, data):
    return _gunzip(eng.L, lambda out, n, taken: eng.L.pf_gunzip_device_bgzf(eng.ctx, data, len(data), out, n, taken))


def host_gunzip(eng, data):
    return _gunzip(eng.L, lambda out, n, taken: eng.L.pf_gunzip_host_model_bgzf(data, len(data), out, n, taken))


def device_gzip(eng, data, flags):
    return _text(eng.L, lambda out, n: eng.L.pf_gzip_device(eng.ctx, data, len(data), flags, out, n))


def host_gzip(eng, data, flags):
    return _text(eng.L, lambda out, n: eng.L.pf_gzip_host_model(data, len(data), flags, out, n))


# ---- the decoder
def test_accepted_files_give_their_text(eng):
    bad = []
    for name, data, text in bc.accepted(chunk_bytes()):
        got, why = device_gunzip(eng, data)
        if got != text or host_gunzip(eng, data) != (text, ""):
            bad.append(f"{name}: {why or 'another text'}")
    assert not bad, bad
    ms = C.c_float()
    assert eng.L.pf_gunzip_device_last_ms(eng.ctx, C.byref(ms)) == 0 and ms.value > 0


def test_refused_files_are_not_taken_and_leave_nothing_behind(eng):
    """the host model's member and reason, and a good file right after every refusal"""
    good_name, good, good_text = next(i for i in bc.accepted(chunk_bytes()) if i[0] == "tsv_300k_level6")
    bad = []
    for name, data, member, reason in bc.refused(chunk_bytes()):
        got, why = device_gunzip(eng, data)
        _, host_why = host_gunzip(eng, data)
        if got is not None or why.split("not taken: ")[-1] != host_why.split("not taken: ")[-1] or not why.endswith(f"member {member}: {reason}"):
            bad.append(f"{name}: {'taken' if got is not None else why}")
        if device_gunzip(eng, good) != (good_text, ""):
            bad.append(f"{name}: the next call failed")
    assert not bad, bad


def test_the_plain_entry_point_still_refuses_bgzf(eng):
    data = next(d for n, d, _ in bc.accepted(chunk_bytes()) if n == "one_member_1")
    got, why = _gunzip(eng.L, lambda out, n, taken: eng.L.pf_gunzip_device(eng.ctx, data, len(data), out, n, taken))
    assert got is None and why.endswith("member 0: bad header")


# ---- the encoder
def _sizes(C_):
    return {"0": 0, "1": 1, "C-1": C_ - 1, "C+1": C_ + 1, "3C+17": 3 * C_ + 17}


def _framed(plain_member):
    """a plain member of the encoder's as the BGZF member it must become: FLG = 4, the BC subfield, the rest as it is"""
    return plain_member[:3] + b"\x04" + plain_member[4:10] + struct.pack("<H2sHH", 6, b"BC", 2, len(plain_member) + 8 - 1) + plain_member[10:]


@pytest.mark.parametrize("n", ["0", "1", "C-1", "C+1", "3C+17"])
def test_framed_members_equal_the_host_model_s(eng, n):
    """Under PF_GZ_BGZF the device's bytes are the host model's wherever the two encoders' bytes are equal without it (the
    host model's matcher is a serial one: include/panfeed_hip.h does not promise equal bytes under the product flags, so
    there the frame is compared: every member is the unflagged device member behind the 18-byte head), and the file
    round-trips through the device decoder."""
    from panfeed_amd import _lib
    C_ = chunk_bytes()
    text = dc.real_shapes(C_)["kmers_to_hashes"][:_sizes(C_)[n]]
    for hook in (0, _lib.GZ_FIXED_ONLY, _lib.GZ_DYNAMIC_ONLY, _lib.GZ_LITERALS_ONLY):
        plain, framed = device_gzip(eng, text, hook), device_gzip(eng, text, hook | _lib.GZ_BGZF)
        model_plain, model = host_gzip(eng, text, hook), host_gzip(eng, text, hook | _lib.GZ_BGZF)
        print(f"{n} flags {hook}: device == host model: {plain == model_plain} / framed {framed == model}")
        assert (framed == model) == (plain == model_plain)
        if hook == _lib.GZ_LITERALS_ONLY:
            assert framed == model
        members = bc.walk(framed + bc.EOF)
        assert b"".join(t for _, _, t in members) == text and len(members) == -(-len(text) // C_) + 1
        at_plain = 0
        for off, size, _ in members[:-1]:
            assert framed[off:off + size] == _framed(plain[at_plain:at_plain + size - 8])
            at_plain += size - 8
        assert at_plain == len(plain)
        assert device_gunzip(eng, framed + bc.EOF) == (text, "") and device_gunzip(eng, framed) == (text, "")


def test_framed_segments(eng):
    """three segments, one of them empty: member_end[] in framed offsets, no member across a segment end"""
    from panfeed_amd import _lib
    C_ = chunk_bytes()
    rows = dc.real_shapes(C_)["kmers_to_hashes"]
    parts = [rows[:C_ + 9], b"", rows[C_ + 9:C_ + 700]]
    text = b"".join(parts)
    ends = (C.c_uint64 * 3)(len(parts[0]), len(parts[0]), len(text))
    got = {}
    for who in ("device", "host"):
        out, n, member_end = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 3)()
        if who == "device":
            rc = eng.L.pf_gzip_device_segments(eng.ctx, text, len(text), ends, 3, _lib.GZ_BGZF | _lib.GZ_LITERALS_ONLY, C.byref(out), C.byref(n), member_end)
        else:
            rc = eng.L.pf_gzip_host_model_segments(text, len(text), ends, 3, _lib.GZ_BGZF | _lib.GZ_LITERALS_ONLY, C.byref(out), C.byref(n), member_end)
        _lib.check(rc)
        got[who] = (C.string_at(out, n.value), list(member_end))
        eng.L.pf_free_text(out)
    assert got["device"] == got["host"]
    data, member_end = got["device"]
    assert member_end[0] == member_end[1] and member_end[2] == len(data)
    assert bc.walked_text(data[:member_end[0]] + bc.EOF) == parts[0] and bc.walked_text(data[member_end[1]:] + bc.EOF) == parts[2]
    assert device_gunzip(eng, data) == (text, "")


# ---- the feed's four owners
def _bgzf_block(text):
    """bgzip's block where the table has five of them, else a fifth of the table: at least five members of text"""
    return min(bc.BLOCK, len(text) // 5 + 1)


def _rowfilter_owner():
    from panfeed_amd.downstream import RowFilter
    header, rows = b"cluster\tk-mer\thashed_pattern\n", dc.real_shapes(chunk_bytes())["kmers_to_hashes"]
    lines = rows.split(b"\n")
    keys = sorted({lines[0].split(b"\t")[-1], lines[-1].split(b"\t")[-1], lines[len(lines) // 2].split(b"\t")[-1]})

    def run(path, block, route):
        f = RowFilter(keys, first_field=False)
        try:
            return f.filter_file(path, block_bytes=block, device_gunzip=route)
        finally:
            f.close()
    return RowFilter, header + rows, run, 1


def _assoc_owner():
    from panfeed_amd.downstream import AssocFilter
    text = at.seeded_table(5, skew=len(at.HEADER))

    def run(path, block, route):
        f = AssocFilter(at.PVALUE_FIELD, 8, 1e-8)
        try:
            kept = f.filter_file(path, block_bytes=block, device_gunzip=route)
            cols = f.columns()
            return kept, cols["flags"], cols["rows"], cols["kept"], cols["classes"]
        finally:
            f.close()
    return AssocFilter, text, run, 1


def _kmerjoin_owner():
    import test_gpu_kmerjoin as kjt
    from panfeed_amd.downstream import KJ_RAW, KmerJoin
    header, body = kjt._tile_end_table()

    def run(path, block, route):
        kj = KmerJoin([(b"sel", 0), (b"oth", 1)], 2, [(b"sel", b"ACG")], [b"t0"], [b"t1.0"], b"")
        try:
            got = [kj.survey_file(path, block_bytes=block, device_gunzip=route)]
            for mode in (0, KJ_RAW):
                out = []
                kj.join_file(path, 0, mode, lambda piece: out.append(bytes(piece)), block_bytes=block)
                got.append(b"".join(out))
            return got
        finally:
            kj.close()
    return KmerJoin, header + body, run, 3          # (the survey's pass and two joins' passes)


def _grid_owner():
    import test_gpu_plot_members as pm
    from panfeed_amd.plot import GridBuilder

    def run(path, block, route):
        gb = pm._builder(path, block, route)
        try:
            return pm._snapshot(gb)
        finally:
            gb.close()
    return GridBuilder, pm.tt.PLOT_HEADER + pm.TEXTS["straddle"](), run, 1


OWNERS = {"rowfilter": _rowfilter_owner, "assocfilter": _assoc_owner, "kmerjoin": _kmerjoin_owner, "gridbuilder": _grid_owner}


@pytest.fixture(scope="module", params=sorted(OWNERS))
def owner(request, tmp_path_factory):
    """(the owner's class, its run(path, block_bytes, device_gunzip), passes a run makes, the BGZF file, one whose fourth
    member has a second extra subfield, one with that member's CRC flipped, what the host route gives)"""
    cls, text, run, passes = OWNERS[request.param]()
    d = tmp_path_factory.mktemp(request.param)
    good, foreign, damaged = str(d / "table.tsv.gz"), str(d / "foreign.tsv.gz"), str(d / "damaged.tsv.gz")
    data = bc.make(text, 6, block=_bgzf_block(text))
    members = bc.walk(data)
    assert len(members) >= 6 and gzip.decompress(data) == text
    off, size, _ = members[3]
    with open(good, "wb") as fh:
        fh.write(data)
    with open(damaged, "wb") as fh:
        fh.write(data[:off + size - 8] + bytes([data[off + size - 8] ^ 1]) + data[off + size - 7:])
    with open(foreign, "wb") as fh:
        m = data[off:off + size]
        fh.write(data[:off] + m[:10] + struct.pack("<H2sHH2sHH", 12, b"BC", 2, size + 6 - 1, b"XY", 2, 7) + m[18:] + data[off + size:])
    for path in (foreign,):
        assert gzip.open(path, "rb").read() == text
    return cls, run, passes, good, foreign, damaged, run(good, None, False)


@pytest.mark.parametrize("block", [None, 70000, 5000], ids=["one_read", "reads_of_70000", "reads_of_5000"])
def test_owners_take_bgzf_by_the_device_route(eng, owner, block):
    """whole, and in reads of 70 000 and 5 000 compressed bytes: members straddle reads, a line is carried across calls"""
    cls, run, passes, good, _, _, expected = owner
    before = (cls.device_gunzip_files, cls.fallback_files)
    assert run(good, block, None) == expected                       # the automatic mode
    assert (cls.device_gunzip_files, cls.fallback_files) == (before[0] + passes, before[1])
    assert run(good, block, True) == expected


@pytest.mark.parametrize("block", [None, 5000], ids=["one_read", "reads_of_5000"])
def test_a_member_the_device_refuses_falls_back_or_raises(eng, owner, block):
    """A fourth member that gzip reads and the device decoder does not take (a second extra subfield): the automatic mode
    begins on the device and reads the file again through gzip, to the same result; device_gunzip=True raises.
    A flipped CRC32 in that member is refused by both: the device names the member and the check, and what the automatic
    mode falls back to is gzip's own refusal -- no route hands out rows of a damaged file."""
    from panfeed_amd.downstream import NotTaken
    cls, run, passes, _, foreign, damaged, expected = owner
    before = (cls.device_gunzip_files, cls.fallback_files)
    assert run(foreign, block, None) == expected
    assert (cls.device_gunzip_files, cls.fallback_files) == (before[0], before[1] + 1)
    with pytest.raises(NotTaken) as e:
        run(foreign, block, True)
    assert "bad header" in str(e.value)
    with pytest.raises(NotTaken) as e:
        run(damaged, block, True)
    assert "CRC32 differs" in str(e.value) and ("member 3" in str(e.value) or block)
    before = (cls.device_gunzip_files, cls.fallback_files)
    with pytest.raises((OSError, zlib.error)):                       # (gzip.BadGzipFile, from whichever reader the host route has)
        run(damaged, block, None)
    assert (cls.device_gunzip_files, cls.fallback_files) == (before[0], before[1] + 1)


# ---- end to end
def test_panfeed_bgzf_files_and_the_downstream_tool(tmp_path, monkeypatch):
    """the smallest pangenome of the command's golden chain: --gpu-compress --bgzf writes three BGZF files that decompress to
    the plain run's, and panfeed-get-clusters reads them by the device route"""
    from panfeed_amd import cli, downstream
    from test_gpu_cli import materialise
    golden = json.load(gzip.open(os.path.join(REPO, "tests", "golden", "cli.json.gz"), "rt"))
    ch = golden["chain"]
    materialise(golden["pangenomes"][ch["pangenome"]], str(tmp_path))
    monkeypatch.chdir(tmp_path)
    assert cli.main(ch["pass1_args"] + ["-o", "pass1", "--gpu-compress", "--bgzf"]) == 0
    assert sorted(os.listdir("pass1")) == sorted(name + ".gz" for name in ch["pass1"])
    for name, text in ch["pass1"].items():
        with open(os.path.join("pass1", name + ".gz"), "rb") as fh:
            data = fh.read()
        members = bc.walk(data)
        assert b"".join(t for _, _, t in members).decode() == text and gzip.decompress(data).decode() == text, name
        assert all(len(t) <= bc.BLOCK for _, _, t in members)
    with open("assoc.tsv", "w") as fh:
        fh.write(ch["associations"])
    before = (downstream.RowFilter.device_gunzip_files, downstream.RowFilter.fallback_files)
    out = io.StringIO()
    argv = [a + ".gz" if a.startswith("pass1/") else a for a in ch["clusters_args"]]
    assert downstream.get_clusters(argv, out=out) == 0
    assert sorted(out.getvalue().splitlines()) == sorted(ch["clusters_stdout"].splitlines())
    assert (downstream.RowFilter.device_gunzip_files, downstream.RowFilter.fallback_files) == (before[0] + 1, before[1])
