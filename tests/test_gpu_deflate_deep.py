"""The device gzip encoder's second effort level on the GPU (PF_GZ_DEEP; gz_encode_kernel<true>, csrc/pf_deflate.hip) on the
edge texts of tests/deflate_deep_model.py: every output decodes to its input, its tokens are exactly the rule's
(parse_device_deep), the block type is the smallest and the codes complete; the same text gives the same bytes; level 2
is no larger than level 1 and than zlib's level ZLIB_LEVEL where the host model was; the chunks a workgroup encodes one
after the other come out as each does alone; the device inflater takes the members; run_files and panfeed-get-kmers
write files at level 2 that read back as the plain text."""
import ctypes as C
import gzip
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_cases as dc  # noqa: E402
import deflate_deep_model as dd  # noqa: E402
import deflate_tokens as dt  # noqa: E402

pytestmark = pytest.mark.gpu

FILES = ("kmers.tsv", "kmers_to_hashes.tsv", "hashes_to_patterns.tsv")


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


def device_gzip_segments(eng, data, ends, flags):
    from panfeed_amd import _lib
    out, n = C.c_void_p(), C.c_uint64()
    seg = (C.c_uint64 * len(ends))(*ends)
    member_end = (C.c_uint64 * len(ends))()
    _lib.check(eng.L.pf_gzip_device_segments(eng.ctx, data, len(data), seg, len(ends), flags, C.byref(out), C.byref(n), member_end))
    try:
        return (C.string_at(out, n.value) if n.value else b""), list(member_end)
    finally:
        eng.L.pf_free_text(out)


def device_gunzip(eng, members, bgzf=False):
    from panfeed_amd import _lib
    out, n, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    fn = eng.L.pf_gunzip_device_bgzf if bgzf else eng.L.pf_gunzip_device
    _lib.check(fn(eng.ctx, members, len(members), C.byref(out), C.byref(n), C.byref(taken)))
    try:
        return taken.value, (C.string_at(out, n.value) if n.value else b"")
    finally:
        eng.L.pf_free_text(out)


def chunk_bytes():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


@pytest.fixture(scope="module")
def audits(eng):
    """every deep case encoded under DEEP with each forced block type and decoded to tokens, once"""
    C_ = chunk_bytes()
    return {name: dd.audit_deep(name, data, lambda d, f: device_gzip(eng, d, f | dd.DEEP), dd.parse_device_deep, C_)
            for name, data in dd.deep_cases(C_)}


def test_every_case_decodes_to_the_input_and_gives_the_same_bytes_twice(eng):
    C_ = chunk_bytes()
    bad = []
    for name, data in dd.deep_cases(C_):
        for flags in dd.DEEP_FLAGS:
            try:
                members = device_gzip(eng, data, flags)
                dc.check_members(data, members, C_)
                assert device_gzip(eng, data, flags) == members, "the same text gave other bytes the second time"
            except Exception as e:      # noqa: BLE001  (every failing case is named, not only the first)
                bad.append((name, flags, type(e).__name__, str(e)[:80]))
    assert not bad, bad


def test_tokens_block_choice_and_codes_of_every_case(audits):
    bad = [b for failures, _ in audits.values() for b in failures]
    assert not bad, (len(bad), bad[:20])


def test_cases_of_level_1_under_the_deep_rule(eng):
    """the cases of deflate_cases.cases too: lengths and distances at every symbol's edge, runs, ragged chunks"""
    C_ = chunk_bytes()
    bad = []
    for name, data, _ in dc.cases(C_):
        if name.startswith("shape_"):           # (among the deep cases already)
            continue
        bad += dd.audit_deep(name, data, lambda d, f: device_gzip(eng, d, f | dd.DEEP), dd.parse_device_deep, C_)[0]
    assert not bad, (len(bad), bad[:20])


def test_what_the_cases_were_built_for(audits):
    """computed from the kernel's own tokens: symbol 257 from the near 3-byte agreement and not from the far one, the
    match over MAX_MATCH at distance 301, the deferrals at a step's last position, at two steps' and in a chain"""
    tok = {name: [m.tokens for m in decoded[0]] for name, (_, decoded) in audits.items()}
    assert (3, 4096) in tok["three_bytes_near"][0]
    assert not any(not isinstance(t, int) and t[0] == 3 for t in tok["three_bytes_far"][0])
    at = tok["equal_rows_300"][0].index((258, 301))
    assert tok["equal_rows_300"][0][at + 1][1] == 301
    cases = dict(dd.deep_cases(chunk_bytes()))
    for name, at in (("lazy_at_255", (255,)), ("lazy_at_511", (511,)), ("lazy_chain", (300, 301, 302)),
                     ("lazy_through_b_at_255", (255,)), ("lazy_through_b_at_511", (511,)),
                     ("lazy_at_n_minus_2", (len(cases["lazy_at_n_minus_2"]) - 5,))):
        got = dd.deferrals(cases[name], dd.parse_device_deep)
        assert all(q in got for q in at), (name, got)
        assert tok[name][0] == dd.parse_device_deep(cases[name])
    # the texts of rows: the kernel's tokens are the rule's (the audit), which no kernel gives that overlooks a newline at
    # a step's or a wave's edge, carries the wrong second-to-last one, or takes B a byte off (the host test shows that
    # the rule's tokens differ from each of those); here, that they are not level 1's
    for name in ("long_rows", "unequal_rows") + tuple(f"newline_at_{at}" for at in (63, 64, 191, 192, 255, 256, 257)):
        assert tok[name][0] == dd.parse_device_deep(cases[name]) != dt.parse_device(cases[name]), name
    assert tok["unequal_rows"][0] != dd._deep(cases["unequal_rows"], dd._cands_device(cases["unequal_rows"]), False, "noclause")
    # the second member of C + 1 bytes of equal rows holds one byte: nothing before it
    assert tok["equal_rows_over_a_chunk"][1] == [cases["equal_rows_over_a_chunk"][-1]]


def test_literals_only_wins(eng):
    C_ = chunk_bytes()
    text = dc.real_shapes(C_)["hashes_to_patterns"][:C_ + 77]
    assert device_gzip(eng, text, dd.DEEP | dc.LITERALS_ONLY) == device_gzip(eng, text, dc.LITERALS_ONLY)


def test_chunk_that_starts_inside_a_row(eng):
    C_ = chunk_bytes()
    text, ends = dd.segment_case(C_)
    members, member_end = device_gzip_segments(eng, text, ends, dd.DEEP)
    assert member_end[-1] == len(members)
    at = 0
    for lo, hi, end in zip([0] + ends[:-1], ends, member_end):
        assert members[at:end] == device_gzip(eng, text[lo:hi], dd.DEEP)
        assert [m.tokens for m in dt.members(members[at:end])] == [dd.parse_device_deep(c) for c in dc.chunks_of(text[lo:hi], C_)]
        at = end


@pytest.fixture(scope="module")
def shape_members(eng):
    """the three real shapes at level 1 and 2, plain and BGZF, each encoded twice"""
    C_ = chunk_bytes()
    out = {}
    for shape, text in dc.real_shapes(C_).items():
        for flags in (0, dd.DEEP, dd.BGZF, dd.DEEP | dd.BGZF):
            out[shape, flags] = (device_gzip(eng, text, flags), device_gzip(eng, text, flags))
    return out


def test_same_text_gives_the_same_bytes(shape_members):
    for (shape, flags), (one, two) in shape_members.items():
        assert one == two, (shape, flags)
        assert gzip.decompress(one) == dc.real_shapes(chunk_bytes())[shape], (shape, flags)


@pytest.mark.parametrize("bgzf", [0, dd.BGZF], ids=["plain", "bgzf"])
def test_level_2_sizes(shape_members, bgzf):
    """the host test's two conditions on the device's bytes, against the same zlib level"""
    C_ = chunk_bytes()
    for shape, text in dc.real_shapes(C_).items():
        one, two = len(shape_members[shape, bgzf][0]), len(shape_members[shape, dd.DEEP | bgzf][0])
        z = {level: dd.zlib_total(text, C_, level, 8 if bgzf else 0) for level in (1, 4, 6, 9)}
        print(f"{shape}: {len(text)} bytes of text, level 1 {one}, level 2 {two}, zlib 1/4/6/9 on the same cuts {z}")
        assert two <= one, shape
        if shape == "hashes_to_patterns":
            assert two <= z[dd.ZLIB_LEVEL]


def test_device_inflater_takes_the_members(eng, shape_members):
    text = dc.real_shapes(chunk_bytes())["hashes_to_patterns"]
    assert device_gunzip(eng, shape_members["hashes_to_patterns", dd.DEEP][0]) == (1, text)
    assert device_gunzip(eng, shape_members["hashes_to_patterns", dd.DEEP | dd.BGZF][0], bgzf=True) == (1, text)


def chunk_kinds(C_):
    """whole chunks of the deep cases' kinds"""
    real, cases = dc.real_shapes(C_), dict(dd.deep_cases(C_))

    def whole(text):
        return (text * (C_ // len(text) + 1))[:C_]
    return [("rows", real["hashes_to_patterns"][:C_]), ("only_newlines", b"\n" * C_), ("no_newline", dd._row(11, C_)),
            ("equal_rows", whole(dd.cell_rows(9, 127, 1) * 2)), ("seam_rows", whole(cases["newline_at_255"])), ("long_rows", whole(cases["long_rows"])),
            ("kmers_tsv", real["kmers_tsv"][7:C_ + 7]), ("lazy", whole(cases["lazy_at_255"] + b"\n" + cases["lazy_chain"]))]


def test_chunks_of_one_workgroup_are_encoded_as_each_is_alone(eng):
    """600 whole chunks and a ragged tail, more than one chunk for some of the 512 workgroups of a 256-CU part, eight kinds
    in turn so that the chunks a workgroup meets one after the other differ in kind: every member is, byte for byte, the
    single member of its chunk's text alone -- the newline carry, the walk's look into the next step, the match carried
    past a step do not reach the next chunk"""
    C_ = chunk_bytes()
    kinds = chunk_kinds(C_)
    tail = dc.real_shapes(C_)["hashes_to_patterns"][5:C_ // 3 + 10]
    alone = [device_gzip(eng, text, dd.DEEP) for _, text in kinds]
    tail_alone = device_gzip(eng, tail, dd.DEEP)
    for (name, text), member in zip(kinds, alone):
        (m,) = dt.members(member)
        assert m.text == text, name
    order = [(i + i // 512) % len(kinds) for i in range(600)]
    assert all(order[i] != order[i + 512] for i in range(600 - 512))
    raw = device_gzip(eng, b"".join(kinds[k][1] for k in order) + tail, dd.DEEP)
    sizes = dd.member_sizes(raw)
    assert len(sizes) == 601
    at, bad = 0, []
    for i, (size, want) in enumerate(zip(sizes, [alone[k] for k in order] + [tail_alone])):
        if raw[at:at + size] != want:
            bad.append((i, "tail" if i == 600 else kinds[order[i]][0], size, len(want)))
        at += size
    assert not bad, (len(bad), bad[:10])


# ---- the files
@pytest.fixture(scope="module")
def pangenome(tmp_path_factory):
    from panfeed_amd import synth
    root = tmp_path_factory.mktemp("pg")
    cl = synth.generate(4, 100, first=333, flank=0, mean_len=300, min_len=80, max_len=500, n_rate=0.0, paralog_rate=0.05)
    csvp, _gffs, _fas = synth.write_pangenome(str(root), cl)
    return {"csv": csvp, "gffs": str(root / "gffs"), "targets": (cl[0].names[3],)}


def _run(pg, out, **kw):
    from panfeed_amd.pipeline import run_files
    return run_files(pg["csv"], pg["gffs"], str(out), klength=21, targets=pg["targets"], **kw)


def _device_members(raw):
    """the members the device made, decoded: those with the encoder's own head (the header line's member and any text the
    host compressed carry zlib's)"""
    out, at = [], 0
    for size in dd.member_sizes(raw):
        if raw[at:at + 10] == dt.MEMBER_HEAD:
            out += dt.members(raw[at:at + size])
        at += size
    return out


def test_run_files_at_level_2(pangenome, tmp_path):
    _run(pangenome, tmp_path / "plain")
    st = _run(pangenome, tmp_path / "gz", device_gzip=True, device_gzip_level=2)
    assert sorted(os.listdir(tmp_path / "gz")) == sorted(f + ".gz" for f in FILES)
    for f in FILES:
        assert gzip.decompress((tmp_path / "gz" / (f + ".gz")).read_bytes()) == (tmp_path / "plain" / f).read_bytes(), f
    assert 0 < st["compressed_bytes"] < st["bytes"]
    # the level reached the encoder: the pattern rows' tokens are the deep rule's, which here are not level 1's
    ms = _device_members((tmp_path / "gz" / "hashes_to_patterns.tsv.gz").read_bytes())
    assert ms and all(m.tokens == dd.parse_device_deep(m.text) for m in ms)
    assert any(m.tokens != dt.parse_device(m.text) for m in ms)


def test_run_files_clusters_at_level_2(pangenome, tmp_path):
    _run(pangenome, tmp_path / "plain", multiple_files=True)
    _run(pangenome, tmp_path / "gz", multiple_files=True, device_gzip_clusters=True, device_gzip_level=2)
    dirs = sorted(os.listdir(tmp_path / "plain"))
    assert dirs and sorted(os.listdir(tmp_path / "gz")) == dirs
    deep = 0
    for d in dirs:
        for f in sorted(os.listdir(tmp_path / "plain" / d)):
            raw = (tmp_path / "gz" / d / (f + ".gz")).read_bytes()
            assert gzip.decompress(raw) == (tmp_path / "plain" / d / f).read_bytes(), (d, f)
            if f == "hashes_to_patterns.tsv":
                ms = _device_members(raw)
                assert all(m.tokens == dd.parse_device_deep(m.text) for m in ms)
                deep += sum(m.tokens != dt.parse_device(m.text) for m in ms)
    assert deep


def test_run_files_refuses_another_level(pangenome, tmp_path):
    with pytest.raises(ValueError):
        _run(pangenome, tmp_path / "out", device_gzip=True, device_gzip_level=3)
    assert not (tmp_path / "out").exists()


def test_get_kmers_gz_level_2(tmp_path):
    """panfeed-get-kmers --gz-output --gz-level 2 on a hand-made table (tests/join_tables.py: 60 rows a cluster with long
    notes, a cluster a bunch): the file reads back as the model's text, and the level reached the join's encoder -- among
    the file's members there are some with the deep rule's tokens where the two rules differ and none with level 1's;
    at level 1 the reverse.  (The host's own members, the header line's at least, carry the same 10-byte head: a member
    is told by its tokens.)"""
    import join_tables as jt
    from panfeed_amd import downstream
    t = jt.handmade(rows_per_cluster=60, long_notes=300)
    (tmp_path / "assoc.tsv").write_text(t["assoc"])
    (tmp_path / "kh.tsv").write_bytes(t["kh"])
    (tmp_path / "kmers.tsv").write_bytes(t["kmers"])
    argv = ["-a", str(tmp_path / "assoc.tsv"), "-p", str(tmp_path / "kh.tsv"), "-k", str(tmp_path / "kmers.tsv"), "-t", "0.5",
            "--clusters-per-iteration", "1"]
    model, routes = jt.join_model(str(tmp_path / "assoc.tsv"), t["kh"], t["kmers"], threshold=0.5, per_iteration=1)
    assert all(routes)                                      # (every bunch is one the device joins)
    for level in (1, 2):
        p, out = tmp_path / f"annotated{level}.tsv.gz", io.StringIO()
        assert downstream.get_kmers(argv + ["--gz-output", str(p), "--gz-level", str(level)], out=out) == 0 and out.getvalue() == ""
        assert gzip.decompress(p.read_bytes()).decode() == model
        ms = [m for m in _device_members(p.read_bytes()) if m.tokens is not None]
        deep = [m for m in ms if m.tokens == dd.parse_device_deep(m.text) != dt.parse_device(m.text)]
        plain_rule = [m for m in ms if m.tokens == dt.parse_device(m.text) != dd.parse_device_deep(m.text)]
        assert (deep and not plain_rule) if level == 2 else (plain_rule and not deep), (level, len(ms), len(deep), len(plain_rule))
    assert (tmp_path / "annotated1.tsv.gz").read_bytes() != (tmp_path / "annotated2.tsv.gz").read_bytes()
