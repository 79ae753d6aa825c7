"""The text-table models without a GPU: the case lists of tests/text_tables.py reach every class of the classifier (so
that thinning a list cannot quietly lose an edge), the pure-Python models agree with pandas where pandas reads a table
the same way, the block reader under both scanners (`scan_lines`) shows its consumer every byte once, as does the pass
over a file of gzip members (`pass_member_file`), `route_file` chooses between the two as it says, and the ordered
64-bit keys of the plot grids order doubles as IEEE does."""
import gzip
import io

import numpy as np
import pytest

import text_tables as tt


# ------------------------------------------------------------------------------------------------ models by hand
def test_filter_rows_by_hand():
    text = b"ab\t1\tkey\nabc\t2\tkey2\n\t\tkey\n\nab\nabc\tlast\tkey"
    assert tt.filter_rows(text, [b"key"], False) == b"ab\t1\tkey\n\t\tkey\n"
    assert tt.filter_rows(tt.as_file(text), [b"key"], False) == b"ab\t1\tkey\n\t\tkey\nabc\tlast\tkey\n"
    assert tt.filter_rows(text, [b"ab", b""], True) == b"ab\t1\tkey\n\t\tkey\n\nab\n"
    assert tt.filter_rows(text, [b"ab", b"ab"], False) == b"ab\n"
    assert tt.filter_rows(text, [], True) == b"" and tt.filter_rows(text, [b"ab\t1"], True) == b""
    long = b"x" * 4096
    assert tt.filter_rows(long + b"\t1\n" + long[1:] + b"\t2\n", [long, long[1:]], True) == long[1:] + b"\t2\n"
    # carriage returns and double quotes are ordinary bytes of a field (known difference) ...
    assert tt.filter_rows(b"ab\t1\tk\r\nab\r\t2\tk\n", [b"k\r", b"ab\r"], False) == b"ab\t1\tk\r\n"
    assert tt.filter_rows(b'"ab"\t1\n"a\tb"\t2\nab\t3\n', [b'"ab"', b'"a'], True) == b'"ab"\t1\n"a\tb"\t2\n'


def test_pandas_reads_carriage_returns_and_quotes_otherwise():
    """... where pandas ends a line at a lone carriage return and takes double quotes as quoting"""
    import pandas as pd
    cr = pd.read_csv(io.BytesIO(b"c\tv\nab\t1\rcd\t2\n"), sep="\t", dtype=str)
    assert cr["c"].tolist() == ["ab", "cd"]
    assert tt.lines_of(b"ab\t1\rcd\t2\n") == [b"ab\t1\rcd\t2"]
    q = pd.read_csv(io.BytesIO(b'c\tv\n"a\tb"\t2\n'), sep="\t", dtype=str)
    assert q["c"].tolist() == ["a\tb"]
    assert tt.lines_of(b'"a\tb"\t2\n')[0].split(b"\t")[0] == b'"a'


def test_plot_model_by_hand():
    text = (b"g\ts1\t5\tacgT\t1\tp1\n" b"g\ts1\t5\tacgT\t-1.0\tp2\n" b"g\ts2\t-3\t\t-1\tp1\n" b"g\tzz\t0\tA\t1\tp9\n"
            b"\n" b"h\ts1\tabc\tA\t1\tp3\n" b"h\ts1\n" b"g\ts1\t+7\tNNx\t-01\tp1\textra\n" b"\t\t\t\t\t\n")
    m = tt.plot_model(text, tt.PLOT_COLUMNS, [b"s1", b"s2", b"s1"])
    assert m.clusters == {b"g": (-3, 7, 4), b"h": (None, None, 0)}
    assert m.cells == {(b"g", 0, 5): tt.Cell(2, [ord("A"), ord("A")], {b"p1", b"p2"}),
                       (b"g", 1, -3): tt.Cell(1, [0], {b"p1"}), (b"g", 0, 7): tt.Cell(1, [ord("N")], {b"p1"})}
    assert m.texts == {b"p1", b"p2"} and m.lines == 8 and m.records == 4
    z = tt.plot_model(text, tt.PLOT_COLUMNS, [b"s1", b"s2"], 5, 5)
    assert z.clusters == {b"g": (5, 5, 2), b"h": (None, None, 0)} and z.records == 2 and z.texts == {b"p1", b"p2"}
    assert tt.plot_model(text, tt.PLOT_COLUMNS, [b"s1"], 6, 4).records == 0
    for pos, ok in ((b"2147483647", True), (b"-2147483647", True), (b"2147483648", False), (b"-2147483648", False)):
        row = b"g\ts1\t" + pos + b"\tA\t1\tp\n"
        if ok:
            assert tt.plot_model(row, tt.PLOT_COLUMNS, [b"s1"]).records == 1
        else:
            with pytest.raises(tt.ModelArgumentError):
                tt.plot_model(row, tt.PLOT_COLUMNS, [b"s1"])
    assert [tt.letter_of(b"acgt", s) for s in (b"-1", b"-1.0", b"-01", b"1", b"+1", b"0", b"-11", b"", b"-")] == \
        [ord(c) for c in "AAAAAAAAA"]
    assert [tt.letter_of(b"tgcA", s) for s in (b"-1", b"-1.0", b"-01", b"1", b"-11", b"", b"-")] == [ord(c) for c in "TTTTTTT"]
    assert [tt.letter_of(k, b"-1") for k in (b"a", b"c", b"g", b"t", b"n", b"ACx", b"")] == [ord(c) for c in "TGCANN"] + [0]
    assert [tt.letter_of(k, b"1") for k in (b"n", b"xA", b"")] == [ord("N"), ord("X"), 0]
    assert tt.ieee_max([float("nan"), -0.0, 0.0]) == 0 and np.signbit(tt.ieee_max([-0.0, float("nan")]))
    assert tt.ieee_max([float("nan")]) is None and tt.ieee_max([-np.inf, -5.0]) == -5.0


def test_classifier_by_hand():
    block = b"ab\t1\tk\n\n\t\t\n" + b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFG\tz\n"
    c = tt.line_classes(block, [b"ab", b"abc"], "first")
    assert c[0] == {"end%16=6", "nl_mid", "first_in_block", "field_inside", "key_equal", "field_prefix_of_key"}
    assert c[1] == {"end%16=7", "nl_top", "blank", "field_empty", "field_prefix_of_key"}     # (an empty field is a prefix)
    assert c[2] == {"end%16=10", "nl_mid", "tabs_only", "field_empty", "field_prefix_of_key"}
    assert c[3] == {"end%16=8", "nl_low", "last_in_block", "field_span", "key_prefix_of_field"}
    assert tt.line_classes(block, [b"z"], "last")[3] >= {"field_inside", "key_equal"}
    assert "field_straddle" in tt.line_classes(b"0123456789abcd\tXY\n", [], 1)[0]
    assert not set(tt.FIELD_SPAN + ("field_empty",)) & tt.line_classes(b"a\tb\n", [], 2)[0]
    assert tt.line_classes(b"a\n")[0] >= {"first_in_block", "last_in_block", "alone_in_block", "end%16=1"}
    assert tt.block_classes(b"x" * 31 + b"\n") == {"block%16=0"} and tt.block_classes(b"ab\n") == frozenset()
    assert tt.blocks_of(b"ab\ncd\nefgh", 4) == [b"ab\n", b"cd\n", b"efgh\n"]
    assert tt.blocks_of(b"abcdefgh\n\n", 3) == [b"abcdefgh\n", b"\n"] and tt.blocks_of(b"", 5) == []


# ------------------------------------------------------------------------------------------------ coverage of the lists
def _reached(text, keys, field, sizes):
    """classes over every block the sweep hands to a kernel; and, apart, the classes of the lines a key selects"""
    every, kept, blocks = set(), set(), set()
    for blk in [text] + [b for n in sizes for b in tt.blocks_of(text, n)]:
        blocks |= tt.block_classes(blk)
        for cls in tt.line_classes(blk, keys, field):
            every |= cls
            if "key_equal" in cls:
                kept |= cls
    return every, kept, blocks


@pytest.mark.parametrize("field", ["first", "last"])
def test_rowfilter_alignment_list_reaches_every_class(field):
    text = tt.rowfilter_alignment_text()
    assert 2000 < len(text) < 12000
    every, kept, blocks = _reached(text, tt.RF_KEYS + (b"",), field, tt.BLOCK_SIZES)
    want = set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN + tt.PLACE + tt.KEY_RELATION + tt.OTHER)
    assert want <= every, sorted(want - every)
    # the lines a key selects: every place of the line end, every extent of the field, every place in a block
    want = set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN + tt.PLACE + ("field_empty", "blank", "tabs_only"))
    assert want <= kept, sorted(want - kept)
    assert blocks == set(tt.BLOCK_MOD)
    # and in the one-block scan alone every place of the line end with a line a key selects
    one = set().union(*[c for c in tt.line_classes(text, tt.RF_KEYS, field) if "key_equal" in c])
    assert set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN) <= one, sorted(set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN) - one)


def test_plot_alignment_list_reaches_every_class():
    text = tt.plot_alignment_text()
    assert 2000 < len(text) < 12000
    every, _kept, blocks = _reached(text, (), tt.PLOT_COLUMNS[0], (64, 257))
    want = set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN + tt.PLACE + ("blank", "tabs_only", "field_empty"))
    assert want <= every, sorted(want - every)
    assert blocks == set(tt.BLOCK_MOD)
    one = set().union(*tt.line_classes(text, (), 0))
    assert set(tt.END_MOD + tt.NL_BYTE + tt.FIELD_SPAN) <= one
    m = tt.plot_model(text, tt.PLOT_COLUMNS, tt.PLOT_STRAINS)
    assert {1, 2} <= {c.count for c in m.cells.values()} and max(c.count for c in m.cells.values()) >= 3
    assert any(len(c.texts) > 1 for c in m.cells.values())
    assert m.lines > m.records > 100 and len(m.clusters) == 23


def test_byte_sweeps_put_every_byte_behind_every_place_of_a_newline():
    for text, lo, hi, name in ((tt.rowfilter_byte_sweep_text(), 0, 256, tt.SWEEP_KEY),
                               (tt.plot_byte_sweep_text(), 1, 128, tt.PLOT_NAME)):
        seen, at = set(), 0
        for ln in tt.lines_of(text):
            if at and ln[1:].startswith(name):
                seen.add((ln[0], (at - 1) % 4))
            if at and ln.startswith(b"\x0b") and ln.lstrip(b"\x0b").startswith(name):
                seen.add((len(ln) - len(ln.lstrip(b"\x0b")), "run", (at - 1) % 4))
            at += len(ln) + 1
        assert seen >= {(c, r) for c in range(lo, hi) if c not in (9, 10) for r in range(4)}
        assert seen >= {(n, "run", r) for n in (2, 3) for r in range(4)}
    ends = {ln.split(b"\t")[0][-1] for ln in tt.lines_of(tt.rowfilter_byte_sweep_text()) if ln.startswith(tt.SWEEP_KEY)}
    assert ends == set(range(256)) - {9, 10}


# ------------------------------------------------------------------------------------------------ models against pandas
def _regular(text, n_fields):
    """the lines of `text` with exactly n_fields fields, not all of them empty: what pandas reads as rows of one shape"""
    return b"".join(ln + b"\n" for ln in tt.lines_of(text) if ln.count(b"\t") == n_fields - 1 and ln.strip(b"\t"))


@pytest.mark.parametrize("first_field", [True, False])
def test_filter_rows_equals_pandas_isin(first_field):
    import pandas as pd
    body = _regular(tt.rowfilter_alignment_text(), 3)
    assert body.count(b"\n") > 150
    df = pd.read_csv(io.BytesIO(b"a\tb\tc\n" + body), sep="\t", dtype=str, keep_default_na=False)
    for keys in ([b"ab"], list(tt.RF_KEYS), list(tt.RF_KEYS) + [b""], [b"nope"], []):
        kept = df[df["a" if first_field else "c"].isin([k.decode() for k in keys])]
        exp = kept.to_csv(sep="\t", index=False, header=False).encode()
        assert tt.filter_rows(body, keys, first_field) == exp, keys
    assert tt.filter_rows(body, list(tt.RF_KEYS) + [b""], first_field).count(b"\n") > 60


@pytest.mark.parametrize("zoom", [(None, None), (-2, 3), (4, 4)])
def test_plot_model_equals_pandas_groupby(zoom):
    import pandas as pd
    body = _regular(tt.plot_alignment_text(), 6)
    df = pd.read_csv(io.BytesIO(tt.PLOT_HEADER + body), sep="\t", keep_default_na=False,
                     dtype={"cluster": str, "strain": str, "k-mer": str, "lrt-pvalue": str, "gene_start": int, "strand": int})
    names = [s.decode() for s in tt.PLOT_STRAINS]
    df = df[df["strain"].isin(names)]
    listed = set(df["cluster"])
    if zoom[0] is not None:
        df = df[(df["gene_start"] >= zoom[0]) & (df["gene_start"] <= zoom[1])]
    m = tt.plot_model(body, tt.PLOT_COLUMNS, tt.PLOT_STRAINS, *zoom)
    assert {k.decode() for k in m.clusters} == listed and m.records == len(df) > 0
    by_cluster = df.groupby("cluster")["gene_start"].agg(["min", "max", "size"])
    for name, (mn, mx, rows) in m.clusters.items():
        if rows:
            assert tuple(by_cluster.loc[name.decode()]) == (mn, mx, rows)
        else:
            assert name.decode() not in by_cluster.index
    comp = {"A": "T", "T": "A", "G": "C", "C": "G"}
    up = df["k-mer"].str.upper()
    letter = [0 if not k else ord(comp.get(k[-1], "N") if s == -1 else k[0]) for k, s in zip(up, df["strand"])]
    df = df.assign(letter=letter, sid=[names.index(s) for s in df["strain"]])
    grp = df.groupby(["cluster", "sid", "gene_start"])
    exp = {(c.encode(), s, p): (len(g), g["letter"].tolist(), {t.encode() for t in g["lrt-pvalue"]}) for (c, s, p), g in grp}
    assert {k: (v.count, v.letters, v.texts) for k, v in m.cells.items()} == exp
    assert m.texts == {t.encode() for t in df["lrt-pvalue"]}


# ------------------------------------------------------------------------------------------------ scan_lines
def _shown(fh, block_bytes):
    """what a consumer of complete lines is shown by scan_lines"""
    from panfeed_amd.downstream import scan_lines
    seen = []

    def scan(buf, n):
        cut = bytes(buf[:n]).rfind(b"\n") + 1
        if cut:
            seen.append(bytes(buf[:cut]))
        return cut

    scan_lines(fh, scan, block_bytes)
    return seen


LADDER = b"".join(b"x" * n + b"\n" for n in range(41))


@pytest.mark.parametrize("body", [LADDER, LADDER + b"tail without newline", b"", b"\n", b"one line"], ids=["ladder", "tail", "empty", "blank", "no-newline"])
def test_scan_lines_shows_every_byte_once(body):
    for block in range(1, 41):
        seen = _shown(io.BytesIO(body), block)
        assert b"".join(seen) == tt.as_file(body), block
        assert seen == tt.blocks_of(body, block), block


def test_scan_lines_header_only_long_line_and_gzip(tmp_path):
    from panfeed_amd.downstream import open_table
    fh = io.BytesIO(b"cluster\tk-mer\n")
    assert fh.readline() == b"cluster\tk-mer\n" and _shown(fh, 7) == []
    # a line longer than the buffer's 64 KiB of slack: the buffer grows
    body = b"a\n" + b"L" * 200_000 + b"\nb\tc\n" + b"M" * 70_000
    seen = _shown(io.BytesIO(body), 1024)
    assert b"".join(seen) == body + b"\n" and seen == tt.blocks_of(body, 1024)
    # a .gz file of several members
    p = tmp_path / "t.tsv.gz"
    parts = [LADDER[:100], LADDER[100:101], LADDER[101:500], LADDER[500:] + b"unterminated"]
    p.write_bytes(b"".join(gzip.compress(x) for x in parts))
    for block in (1, 13, 64, 1 << 16):
        with open_table(str(p)) as fh:
            assert b"".join(_shown(fh, block)) == LADDER + b"unterminated\n", block


# ------------------------------------------------------------------------------------------------ the member-file pass
REC = 7                                                       # the stub's "members": records of REC bytes, b"<nnnnn>"
MEMBER_FILE = b"".join(b"<%05d>" % i for i in range(6))


class MemberStub:
    """a stand-in for a device text feed: takes the whole records at the front of a block once it holds `need` of them (or
    the file ends), and keeps what it was shown and what it used up; at call number `refuse_at` it takes nothing"""

    def __init__(self, need=1, refuse_at=None):
        self.need, self.refuse_at = need, refuse_at
        self.begun, self.lasts, self.used, self.after, self.reasons = 0, [], [], 0, 0

    def begin(self):
        assert not self.lasts
        self.begun += 1

    def call(self, data, last):
        self.lasts.append(last)
        if len(self.lasts) == self.refuse_at:
            return 0, False
        whole = len(data) // REC
        if last:
            assert len(data) == whole * REC                    # the end of the file is the end of a record
        used = whole * REC if last or whole >= self.need else 0
        assert all(data[i:i + 1] == b"<" and data[i + REC - 1:i + REC] == b">" for i in range(0, used, REC))
        self.used.append(data[:used])
        return used, True

    def ran_after(self):
        self.after += 1

    def reason(self):
        self.reasons += 1
        return "the stub's reason"

    def run(self, path, block):
        from panfeed_amd.downstream import pass_member_file
        return pass_member_file(path, block, self.begin, self.call, self.ran_after, self.reason)


@pytest.fixture(scope="module")
def member_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("member_file") / "records.gz"
    p.write_bytes(MEMBER_FILE)
    return str(p)


# (REC and 2 * REC put every / every other record boundary exactly at a block's end; 1 and REC - 1 make calls that hold no
# whole record yet, as does every `need` above 1: used == 0, taken, while more of the file remains)
@pytest.mark.parametrize("need", [1, 2, 4])
@pytest.mark.parametrize("block", [1, REC - 1, REC, REC + 1, 2 * REC, len(MEMBER_FILE)])
def test_member_file_pass_shows_every_byte_once(member_file, block, need):
    s = MemberStub(need)
    assert s.run(member_file, block) is True
    assert s.begun == 1 and b"".join(s.used) == MEMBER_FILE and s.reasons == 0
    # read number i is short, and the end of the file known, when i blocks are more than the file
    first_last = len(MEMBER_FILE) // block + 1
    assert s.lasts == [i >= first_last for i in range(1, len(s.lasts) + 1)] and s.lasts[-1] is True
    assert s.after == len(s.lasts)
    if block < REC * need:
        assert b"" in s.used[:-1]                              # some call took nothing yet, and the pass read on


@pytest.mark.parametrize("block", [1, REC, REC + 1, len(MEMBER_FILE)])
@pytest.mark.parametrize("k", [1, 2, "final"])
def test_member_file_pass_stops_at_a_block_not_taken(member_file, block, k):
    whole = MemberStub()
    assert whole.run(member_file, block)
    k = len(whole.lasts) if k == "final" else k
    s = MemberStub(refuse_at=k)
    assert s.run(member_file, block) is False
    assert len(s.lasts) == k and s.reasons == 1 and s.after == k - 1
    assert s.lasts == whole.lasts[:k] and s.used == whole.used[:k - 1]


class RouteStub:
    """the two routes and the owner's counters of a route_file call"""
    device_gunzip_files = fallback_files = 0

    def __init__(self, taken):
        self.taken, self.log = taken, []

    def run(self, path, device_gunzip):
        from panfeed_amd.downstream import route_file
        return route_file(path, device_gunzip, lambda: self.log.append("members") or ("members" if self.taken else None),
                          lambda: self.log.append("host") or "host", self, lambda: self.log.append("again"), lambda: "the stub's reason")

    def counts(self):
        return self.device_gunzip_files, self.fallback_files


def test_route_decision(tmp_path):
    from panfeed_amd.downstream import GZ_HEAD, NotTaken
    device_gz, host_gz, plain = (str(tmp_path / n) for n in ("device.tsv.gz", "host.tsv.gz", "plain.tsv"))
    (tmp_path / "device.tsv.gz").write_bytes(GZ_HEAD + bytes(6))
    (tmp_path / "host.tsv.gz").write_bytes(b"\x1f\x8b\x08\x08" + bytes(6))  # FLG = FNAME: a header the device does not take
    (tmp_path / "plain.tsv").write_bytes(GZ_HEAD + bytes(6))                # the name decides first
    # automatic: the member route where the file looks like one for it; not taken -> undo, host route, one fallback
    r = RouteStub(taken=True)
    assert r.run(device_gz, None) == "members" and r.log == ["members"] and r.counts() == (1, 0)
    r = RouteStub(taken=False)
    assert r.run(device_gz, None) == "host" and r.log == ["members", "again", "host"] and r.counts() == (0, 1)
    for path in (host_gz, plain):
        r = RouteStub(taken=True)
        assert r.run(path, None) == "host" and r.log == ["host"] and r.counts() == (0, 0)
    # forced: whatever the file; not taken -> NotTaken with the reason, and the host route is never called
    r = RouteStub(taken=True)
    assert r.run(plain, True) == "members" and r.log == ["members"] and r.counts() == (1, 0)
    r = RouteStub(taken=False)
    with pytest.raises(NotTaken, match="the stub's reason"):
        r.run(device_gz, True)
    assert r.log == ["members"] and r.counts() == (0, 0)
    # False never calls the member route
    r = RouteStub(taken=True)
    assert r.run(device_gz, False) == "host" and r.log == ["host"] and r.counts() == (0, 0)
    assert RouteStub.device_gunzip_files == 0 and RouteStub.fallback_files == 0   # (the stubs counted on themselves)


# ------------------------------------------------------------------------------------------------ ordered keys
def test_keys_order_doubles_as_ieee_and_round_trip():
    from panfeed_amd.plot import _floats, _keys
    rng = np.random.default_rng(11)
    tiny = np.float64(5e-324)
    big = np.finfo(np.float64).max
    vals = np.concatenate(([np.nan, -np.nan, -0.0, 0.0, np.inf, -np.inf, tiny, -tiny, big, -big, 1.5, -1.5, 2.2250738585072014e-308],
                           rng.integers(0, 1 << 64, 2000, dtype=np.uint64).view(np.float64), rng.normal(size=200)))
    keys = _keys(vals)
    assert keys.dtype == np.uint64
    nan = np.isnan(vals)
    assert np.array_equal(keys == 0, nan) and nan.sum() >= 2
    back = _floats(keys)
    assert np.array_equal(back.view(np.uint64)[~nan], vals.view(np.uint64)[~nan]) and np.isnan(back[nan]).all()
    v, k = vals[~nan], keys[~nan]
    # IEEE order with -0 below +0: by value, ties by the sign bit
    lt = (v[:, None] < v[None, :]) | ((v[:, None] == v[None, :]) & np.signbit(v)[:, None] & ~np.signbit(v)[None, :])
    assert np.array_equal(k[:, None] < k[None, :], lt)
    assert np.array_equal(k[:, None] == k[None, :], v.view(np.uint64)[:, None] == v.view(np.uint64)[None, :])
