"""panfeed-get-kmers' device join (downstream.KmerJoin -> pf_kmerjoin_*): the survey, plan, place and write kernels of
csrc/pf_rowfilter.hip against the host route (--host-join: the reference's pandas statements) and against the model of
tests/join_tables.py.  No expected text comes from the device route itself."""
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_tables as jt  # noqa: E402
from device_gz_files import write_device_gz  # noqa: E402

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}
RUNS = [(f["case"], i) for f in FIX for i, r in enumerate(f["runs"]) if r["tool"] == "get_kmers"]
WORKER_TIMEOUT_S = 240


def _get_kmers(argv):
    from panfeed_amd import downstream
    out = io.StringIO()
    rc = 0
    try:
        rc = downstream.get_kmers(argv, out=out)
    except SystemExit as e:
        rc = int(e.code or 0)
    return out.getvalue(), rc


def _routes():
    from panfeed_amd.downstream import KmerJoin
    return KmerJoin.device_bunches, KmerJoin.host_bunches, KmerJoin.host_runs


def _moved(before):
    return tuple(b - a for a, b in zip(before, _routes()))


def _golden_files(tmp_path, fx, write=None):
    """the fixture's three files; write(path, text bytes) -> path makes each of the two tables (default: plain)"""
    exp = CASES[fx["case"]]["expect"]
    paths = {}
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        if write is None:
            (tmp_path / name).write_text(exp[name])
            paths[name] = str(tmp_path / name)
        else:
            paths[name] = write(str(tmp_path / name), exp[name].encode())
    (tmp_path / "assoc.tsv").write_text(fx["associations"])
    return paths, str(tmp_path / "assoc.tsv")


def _n_bunches(run):
    el = run["stdout"].splitlines()
    n_clusters = len({ln.split("\t")[0] for ln in el[1:]})
    cpi = int(run["args"][run["args"].index("--clusters-per-iteration") + 1]) if "--clusters-per-iteration" in run["args"] else 15
    return n_clusters, cpi


def _same_as_reference(got, run):
    """the comparison of test_gpu_n4.py"""
    gl, el = got.splitlines(), run["stdout"].splitlines()
    assert gl[:1] == el[:1]
    assert sorted(gl[1:]) == sorted(el[1:])
    n_clusters, cpi = _n_bunches(run)
    if n_clusters <= cpi and "--only-passing" not in run["args"]:
        assert got == run["stdout"]


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{i}" for c, i in RUNS])
def test_golden_runs_go_the_device_route(tmp_path, case, i):
    fx = next(f for f in FIX if f["case"] == case)
    run = fx["runs"][i]
    paths, pa = _golden_files(tmp_path, fx)
    argv = ["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-k", paths["kmers.tsv"]] + run["args"]
    before = _routes()
    got, rc = _get_kmers(argv)
    device, host, refused = _moved(before)
    assert rc == run["rc"]
    _same_as_reference(got, run)
    assert host == 0 and refused == 0
    assert (device > 0) == bool(run["stdout"])
    if "--only-passing" in run["args"] and run["stdout"]:
        from panfeed_amd.downstream import KmerJoin
        st = KmerJoin.last_stats
        print(st)
        assert st["rows_written"] == 0 and st["raw_rows"] == st["rows"] - st["unmatched"]
        kmers_rows = len(jt.rows_of(CASES[case]["expect"]["kmers.tsv"].encode()))
        assert (st["rows"] > 0) == (kmers_rows > 0)     # (two of the golden cases have no target strain: kmers.tsv is its header)
        if kmers_rows:
            assert 0 < st["raw_rows"] < st["rows"]      # fewer raw rows came down than the bunches hold
        before = _routes()
        assert _get_kmers(argv + ["--host-join"])[0] == got
        assert _moved(before) == (0, 0, 0)


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


def _write_host_gz(path, text):
    from panfeed_amd.output import ParallelGzipWriter
    w = ParallelGzipWriter(path + ".gz", chunk_bytes=65536)
    w.write(text.decode())
    w.close()
    return path + ".gz"


@pytest.mark.parametrize("how", ["blocks", "host_gz", "device_gz"])
def test_golden_runs_over_small_blocks_and_gzip_inputs(tmp_path, eng, how):
    from panfeed_amd import downstream
    from panfeed_amd.downstream import KmerJoin
    fx = FIX[0]

    def device_gz(path, text):
        cut = text.index(b"\n") + 1
        write_device_gz(eng, path + ".gz", text[:cut], text[cut:])
        return path + ".gz"

    paths, pa = _golden_files(tmp_path, fx, {"blocks": None, "host_gz": _write_host_gz, "device_gz": device_gz}[how])
    old = downstream.BLOCK_BYTES
    try:
        for blk in (257, 4096) if how == "blocks" else (4096, old):
            downstream.BLOCK_BYTES = blk
            for run in (r for r in fx["runs"] if r["tool"] == "get_kmers" and r["stdout"]):
                before, gz_before = _routes(), (KmerJoin.device_gunzip_files, KmerJoin.fallback_files)
                got, rc = _get_kmers(["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-k", paths["kmers.tsv"]] + run["args"])
                assert rc == 0
                _same_as_reference(got, run)
                device, host, refused = _moved(before)
                assert device > 0 and host == 0 and refused == 0, (blk, run["args"])
                st = KmerJoin.last_stats
                if how == "device_gz":
                    assert KmerJoin.device_gunzip_files > gz_before[0] and KmerJoin.fallback_files == gz_before[1]
                    assert st["members_inflated"] > 0 and st["text_bytes_inflated"] >= len(CASES[fx["case"]]["expect"]["kmers.tsv"])
                else:
                    assert KmerJoin.device_gunzip_files == gz_before[0] and st["members_inflated"] == 0
    finally:
        downstream.BLOCK_BYTES = old


FEED_BLOCK = 4096 // 8          # compressed bytes a read: what the device_gz case above makes of its smaller BLOCK_BYTES


@pytest.fixture(scope="module")
def feed_file(tmp_path_factory, eng):
    """the first fixture's kmers.tsv, plain and device-gzipped: (its bytes, the plain path, the .gz path).  Read FEED_BLOCK
    compressed bytes at a time a member straddles calls, and the members' cut lies inside a line"""
    from device_gz_files import member_sizes
    text = CASES[FIX[0]["case"]]["expect"]["kmers.tsv"].encode()
    d = tmp_path_factory.mktemp("feed")
    plain, gz = str(d / "kmers.tsv"), str(d / "kmers.tsv.gz")
    with open(plain, "wb") as fh:
        fh.write(text)
    cut = text.index(b"\n") + 1
    write_device_gz(eng, gz, text[:cut], text[cut:])
    chunk = eng.L.pf_gzip_device_chunk_bytes()
    with open(gz, "rb") as fh:
        sizes = member_sizes(fh.read())
    assert len(sizes) >= 3 and max(sizes) > 2 * FEED_BLOCK and len(text) > cut + chunk and text[cut + chunk - 1:cut + chunk] != b"\n"
    return text, plain, gz


def _feed_counts(st):
    return st["members_inflated"], st["text_bytes_inflated"]


def test_the_row_filter_and_the_join_run_the_same_feed(feed_file):
    """one process, the two owners of a device text feed by turns over the same member file: the same members and text
    bytes inflated a pass, all of the file's, and the same header line peeled off"""
    import ctypes as C
    from panfeed_amd import _lib
    from panfeed_amd.downstream import KmerJoin, RowFilter
    text, _plain, gz = feed_file
    header = text[:text.index(b"\n") + 1]
    cluster = text[len(header):].split(b"\t", 1)[0]
    rf, kj = RowFilter([cluster], first_field=True), KmerJoin([(cluster, 0)], 1, [], [], [], b"")
    try:
        seen = [_feed_counts(rf.stats()), _feed_counts(kj.stats())]
        for _turn in range(2):
            got_header, rows = rf.filter_file(gz, block_bytes=FEED_BLOCK, device_gunzip=True)
            assert got_header == header and rows and all(ln.split(b"\t", 1)[0] == cluster for ln in rows.splitlines())
            plan = kj.survey_file(gz, block_bytes=FEED_BLOCK, device_gunzip=True)
            assert plan[0]["rows"] == len(rows.splitlines())
            line, n = C.c_void_p(), C.c_uint64()
            _lib.check(kj.L.pf_kmerjoin_members_header(kj.h, C.byref(line), C.byref(n)))
            assert C.string_at(line, n.value) == header
            now = [_feed_counts(rf.stats()), _feed_counts(kj.stats())]
            passes = [tuple(b - a for a, b in zip(before, after)) for before, after in zip(seen, now)]
            print(passes)
            assert passes[0] == passes[1] and passes[0][0] >= 3 and passes[0][1] == len(text)
            seen = now
            _lib.check(kj.L.pf_kmerjoin_reset_counters(kj.h))
    finally:
        rf.close()
        kj.close()


def test_a_join_without_clusters_or_keys_surveys_by_both_routes(feed_file):
    """the join's handle is a feed and its own tables, nothing of a row filter: with no cluster and no key it reads the whole
    file either way and finds no row"""
    from panfeed_amd.downstream import KmerJoin
    text, plain, gz = feed_file
    body = len(text) - (text.index(b"\n") + 1)
    kj = KmerJoin([], 0, [], [], [], b"")
    try:
        scanned = 0
        for path, route in ((gz, True), (plain, False), (gz, False)):
            plan = kj.survey_file(path, block_bytes=FEED_BLOCK if route else 4096, device_gunzip=route)
            assert plan == [{"rows": 0, "unmatched": 0, "bytes": (0, 0), "flags": 0}], (path, route)
            st = kj.stats()
            assert st["bytes_scanned"] - scanned == body, (path, route)
            scanned = st["bytes_scanned"]
        assert st["members_inflated"] >= 3 and st["text_bytes_inflated"] == len(text) and st["rows_written"] == 0
    finally:
        kj.close()


def _handmade_files(tmp_path, t):
    (tmp_path / "assoc.tsv").write_text(t["assoc"])
    (tmp_path / "kh.tsv").write_bytes(t["kh"])
    (tmp_path / "kmers.tsv").write_bytes(t["kmers"])
    return ["-a", str(tmp_path / "assoc.tsv"), "-p", str(tmp_path / "kh.tsv"), "-k", str(tmp_path / "kmers.tsv")]


def _against_model_and_host(tmp_path, t, args, threshold=0.5, per=15):
    """the device route's text; it equals the model's and the host route's, and the bunches went the way the model says"""
    argv = _handmade_files(tmp_path, t) + ["-t", str(threshold), "--clusters-per-iteration", str(per)] + args
    model, routes = jt.join_model(str(tmp_path / "assoc.tsv"), t["kh"], t["kmers"], threshold=threshold, per_iteration=per,
                                  only_passing="--only-passing" in args)
    before = _routes()
    got, rc = _get_kmers(argv)
    moved = _moved(before)
    host, rc_host = _get_kmers(argv + ["--host-join"])
    assert rc == 0 == rc_host
    assert got == model
    assert got == host
    assert moved == (sum(routes), len(routes) - sum(routes), 0)
    return got, routes


@pytest.mark.parametrize("per", [1, 2, 15])
@pytest.mark.parametrize("int_column", [False, True], ids=["text_columns", "int_column"])
@pytest.mark.parametrize("args", [[], ["--only-passing"]], ids=["right", "left"])
def test_handmade_table(tmp_path, per, int_column, args):
    """rows at every offset of a vector, a last row without its newline, clusters and k-mers that are prefixes of one
    another, a k-mer under another cluster only, bunches with every / no row unmatched, both renderings, more than 256
    rows in a block with texts of 0 to 300 bytes"""
    t = jt.handmade(int_column=int_column)
    assert not t["kmers"].endswith(b"\n") and len(jt.rows_of(t["kmers"])) > 256
    assert jt.vector_places(t["kmers"]) == (set(range(16)), set(range(16)))
    got, routes = _against_model_and_host(tmp_path, t, args, per=per)
    assert all(routes) and len(routes) == {1: 6, 2: 3, 15: 1}[per]
    from panfeed_amd.downstream import KmerJoin
    st = KmerJoin.last_stats
    rows = len(got.splitlines()) - 1
    if args:
        assert st["rows_written"] == 0 and 0 < st["raw_rows"] == st["rows"] - st["unmatched"]
    else:      # selected and absent from kmers.tsv: no row; every written row is counted, the unmatched ones as such
        assert st["rows_written"] == rows == st["rows"] and st["unmatched_written"] == st["unmatched"] > 0


def test_handmade_table_in_many_blocks(tmp_path):
    """blocks of 300 bytes: every row is a block's first or last at some point, and rows are carried over"""
    from panfeed_amd import downstream
    old = downstream.BLOCK_BYTES
    try:
        downstream.BLOCK_BYTES = 300
        _against_model_and_host(tmp_path, jt.handmade(rows_per_cluster=20), [], per=2)
    finally:
        downstream.BLOCK_BYTES = old


TILE, SPAN = 1 << 16, 256      # bytes of the text a workgroup and a thread of the join's plan and place kernels own


def _tile_end_table():
    """kmers.tsv of about 200 KB: rows of cluster `sel` (bunch 0; its k-mer ACG is a key, TTT is not) placed by the byte among
    rows of `oth` (bunch 1) and `zz` (not selected).  The plain route's block is the body and the member route's the whole
    file, so every placement is made twice, for a block that starts 0 and len(header) bytes in front of the body"""
    head = len(jt.KMERS_HEADER)
    rows, at = [], 0

    def put(cluster, length=None):                   # a row, of exactly `length` bytes with its newline if given
        nonlocal at
        i = len(rows)
        row = jt.kmers_row(cluster, "ACG" if i % 2 else "TTT", i, strain="s" if length else None)
        if length:
            row = jt.kmers_row(cluster, "ACG" if i % 2 else "TTT", i, strain="s" * (length - len(row)))
        rows.append(row)
        at += len(row) + 1

    def fill_to(target):                             # rows of the other bunch and of no bunch, up to exactly `target`
        while at < target:
            put(("oth", "zz")[len(rows) % 2], None if target - at >= 400 else target - at)
        assert at == target

    for _ in range(3):                               # three rows of the bunch in the first thread's 256 bytes
        put("sel")
    # at a multiple of 256, of 16 and of 4, each for the block that is the body and for the one with the header in front
    for target in (4096, 8192 - head, 12288 + 16, 16384 + 16 - head, 20480 + 4, 24576 + 4 - head):
        fill_to(target)
        put("sel")
    fill_to(TILE - 150)
    put("sel", 150)                                  # ends at the first tile end: behind the header it straddles it
    put("sel")                                       # starts at it
    fill_to(2 * TILE - head)
    put("sel", 150)                                  # behind the header it starts at the second tile end; alone it straddles it
    fill_to(3 * TILE + 1000)                         # (no row of the bunch in the third tile)
    for _ in range(3):
        put("sel")
    return jt.KMERS_HEADER, b"".join(r + b"\n" for r in rows)


def _assert_line_starts(body, shift):
    """the places test_rows_of_a_bunch_at_tile_ends is about, in a block that begins `shift` bytes in front of the body"""
    from collections import Counter
    every, at = [], shift
    for row in body.split(b"\n")[:-1]:
        every.append((at, len(row) + 1, row.startswith(b"sel\t")))
        at += len(row) + 1
    sel = [(b, n) for b, n, mine in every if mine]
    assert ((at + 15) // 16 + 4095) // 4096 == 4                           # four tiles, ends at 65 536, 131 072 and 196 608
    assert any(b % TILE == 0 for b, _ in sel)                              # at a tile end
    assert any(b % SPAN == 0 and b % TILE for b, _ in sel)                 # at the start of a thread's span
    assert any(b % 16 == 0 and b % SPAN for b, _ in sel)
    assert any(b % 4 == 0 and b % 16 for b, _ in sel)
    assert any(b < t < b + n - 1 for b, n in sel for t in (TILE, 2 * TILE, 3 * TILE))       # a tile end in its middle
    # a line is its owner's by the newline in front of it (the block's first by its start)
    own_sel = Counter(max(b - 1, 0) // SPAN for b, _ in sel)
    own_any = {max(b - 1, 0) // SPAN for b, _, _ in every}
    assert max(own_sel.values()) >= 2 and own_any - set(own_sel)
    assert set(range(4)) - {span * SPAN // TILE for span in own_sel}       # a whole tile without a row of the bunch


def test_rows_of_a_bunch_at_tile_ends(tmp_path, eng):
    """One block of four tiles, by both routes and in the three modes: rows of the bunch that start at a tile end, at the
    start of a thread's span, at a multiple of 16 and of 4, one with a tile end in its middle, a thread with three of them,
    threads and a whole tile with none.  The join's place pass puts every row where the plan pass counted it; the text is the
    model's and the same by both routes"""
    from panfeed_amd import _lib
    from panfeed_amd.downstream import KJ_RAW, KmerJoin
    header, body = _tile_end_table()
    for shift in (0, len(header)):
        _assert_line_starts(body, shift)
    plain, gz = str(tmp_path / "kmers.tsv"), str(tmp_path / "kmers.tsv.gz")
    with open(plain, "wb") as fh:
        fh.write(header + body)
    write_device_gz(eng, gz, header, body)
    block = 1 << 18
    assert len(header + body) <= block
    rows, key = jt.rows_of(header + body), (b"sel", b"ACG")
    want = {0: jt.join_rows(rows, {b"sel"}, {key: b"t0"}, b""), 1: jt.join_rows(rows, {b"sel"}, {key: b"t1.0"}, b""),
            KJ_RAW: jt.kept_rows(rows, {b"sel"}, {key})}
    assert 0 < len(want[KJ_RAW]) < len(want[0]) < len(want[1])
    kj = KmerJoin([(b"sel", 0), (b"oth", 1)], 2, [key], [b"t0"], [b"t1.0"], b"")
    try:
        got = {}
        for path, route in ((plain, False), (gz, True)):
            plan = kj.survey_file(path, block_bytes=block, device_gunzip=route)
            assert plan[0]["flags"] == 0 and plan[0]["rows"] == len(want[0].splitlines()) and bool(kj.members[path]) == route
            for mode in (0, 1, KJ_RAW):
                out = []
                kj.join_file(path, 0, mode, lambda piece: out.append(bytes(piece)), block_bytes=block)
                got[route, mode] = b"".join(out)
                assert got[route, mode] == want[mode], (route, mode)
            _lib.check(kj.L.pf_kmerjoin_reset_counters(kj.h))       # (the next survey counts from nothing)
        assert all(got[False, mode] == got[True, mode] for mode in (0, 1, KJ_RAW))
        assert kj.stats()["members_inflated"] >= 4 * 4                    # four passes over the members of four tiles of text
    finally:
        kj.close()


@pytest.mark.parametrize("n", [4095, 4096])
def test_long_fields(tmp_path, n):
    """a strain of 4 095 bytes is a field like any other; one of 4 096 sends its bunch through pandas"""
    t = jt.handmade(rows_per_cluster=6)
    rows = t["kmers"].split(b"\n")
    rows[2] = jt.kmers_row("g", "ACG", 1, strain="s" * n)
    t["kmers"] = b"\n".join(rows)
    _, routes = _against_model_and_host(tmp_path, t, [], per=1)
    assert routes == [n == 4095] + [True] * 5


def test_empty_key_table(tmp_path):
    """the only passing rows of kmers_to_hashes have an empty k-mer: clusters are selected, no key is left, every row
    comes out with empty fields"""
    t = jt.handmade(rows_per_cluster=6)
    t["kh"] = jt.KH_HEADER + b"g\t\tH1\nfull\t\tH5\n"
    got, routes = _against_model_and_host(tmp_path, t, [], per=15)
    assert routes == [True] and len(got.splitlines()) == 13


def test_no_selected_cluster(tmp_path):
    got, routes = _against_model_and_host(tmp_path, jt.handmade(rows_per_cluster=6), [], threshold=1e-30)
    assert got == "" and routes == []


FLAGGED = {jt.TABS: ("g", "s1", "gene", "NODE_1", "1", "5", "36", "0", "31", "1"),
           jt.BYTES: ("g", "caf\u00e9", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.INT: ("g", "s1", "gene", "NODE_1", "1", "007", "36", "0", "31", "1", "ACG"),
           jt.EMPTY: ("g", "s1", "", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.NA: ("g", "NA", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.NUMERIC: ("g", "123", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.WORD: ("g", "s1", "gene", "True", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.LONG: ("g", "s1", "g" * 4096, "NODE_1", "1", "5", "36", "0", "31", "1", "ACG")}


@pytest.mark.parametrize("flag", sorted(FLAGGED), ids=[str(f) for f in sorted(FLAGGED)])
def test_a_flagged_bunch_goes_through_pandas(tmp_path, flag):
    """one row of cluster g sets exactly this flag: that bunch is joined by pandas, the other five by the device, and the
    text is the host route's"""
    row = "\t".join(FLAGGED[flag]).encode()
    assert jt.plainness(row) == flag
    t = jt.handmade(rows_per_cluster=6)
    rows = t["kmers"].split(b"\n")
    rows.insert(3, row)
    t["kmers"] = b"\n".join(rows)
    _, routes = _against_model_and_host(tmp_path, t, [], per=1)
    assert routes == [False] + [True] * 5


def test_out_of_memory_fails_cleanly(tmp_path):
    """pf_debug_limit_alloc below the join's output buffer and above everything else (the row filter's candidate buffer
    over kmers_to_hashes.tsv is 8 MiB; texts of up to 200 000 bytes make the 50 KB of kmers.tsv 13 MB of output): the run
    fails as out of memory, the join closes, and with the limit lifted a fresh run gives the expected text"""
    from panfeed_amd import _lib
    limit = 9 << 20
    t = jt.handmade(long_notes=200000, rows_per_cluster=100)
    argv = _handmade_files(tmp_path, t) + ["-t", "0.5"]
    model, routes = jt.join_model(str(tmp_path / "assoc.tsv"), t["kh"], t["kmers"], threshold=0.5)
    assert routes == [True] and len(model) > limit and 8 * len(t["kmers"]) + 3 * len(t["assoc"]) < limit
    L = _lib.load()
    try:
        _lib.check(L.pf_debug_limit_alloc(limit, None))
        with pytest.raises(_lib.PanfeedHipError) as ei:
            _get_kmers(argv)
        assert ei.value.status == _lib.ERR_OOM
    finally:
        _lib.check(L.pf_debug_limit_alloc(0, None))
    got, rc = _get_kmers(argv)
    assert rc == 0 and got == model


@pytest.fixture(scope="module")
def weak(tmp_path_factory):
    """the weak-hash variant's results: one fresh child with its own time limit, never restarted"""
    out = tmp_path_factory.mktemp("kmerjoin_weakhash")
    try:
        p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "kmerjoin_weakhash_worker.py"), str(out)], capture_output=True,
                           text=True, timeout=WORKER_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        return {"error": f"kmerjoin_weakhash_worker.py did not finish in {WORKER_TIMEOUT_S} s:\n{(e.stderr or b'')[-4000:]}"}
    if p.returncode != 0:
        return {"error": f"kmerjoin_weakhash_worker.py exited with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"}
    with open(os.path.join(str(out), "results.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("mask", ["0x0", "0x7", "0xffffffffffffffff"])
def test_keys_are_verified_by_bytes_under_a_weak_hash(weak, tmp_path, mask):
    """with the text site's hash masked to nothing or to three bits, every look-up meets other clusters' and keys' slots:
    the bytes decide, the text is the shipped library's, and the join counts the compares that failed; with the hash
    whole it counts none"""
    if "error" in weak:
        pytest.fail(weak["error"], pytrace=False)
    t = jt.handmade()
    argv = _handmade_files(tmp_path, t) + ["-t", "0.5", "--clusters-per-iteration", "2"]
    shipped, rc = _get_kmers(argv)
    from panfeed_amd.downstream import KmerJoin
    assert rc == 0 and KmerJoin.last_stats["hash_rejects"] == 0
    got = weak[mask]
    print(mask, {k: v for k, v in got.items() if k != "text"})
    assert got["text"] == shipped
    assert got["routes"] == [3, 0, 0]
    assert (got["hash_rejects"] > 0) == (mask != "0xffffffffffffffff")
