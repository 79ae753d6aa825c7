"""panfeed-get-kmers --gz-output: the annotated table as a file of small gzip members, the device join's rows compressed
where they were written (pf_kmerjoin_set_gzip, csrc/pf_rowfilter.hip) and host-made text beside them
(output.SmallMemberGzipWriter).  The expected text is the reference's recorded stdout (tests/golden/n4.json.gz), the model of
tests/join_tables.py or the same command's plain stdout, and it is Python's gzip that inflates the file: nothing expected
comes from the encoder."""
import gzip
import io
import json
import os
import sys

import pytest

from conftest import GOLDEN, all_cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_tables as jt  # noqa: E402
from device_gz_files import member_sizes  # noqa: E402
from inflate_cases import slot_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}
RUNS = [(f["case"], i) for f in FIX for i, r in enumerate(f["runs"]) if r["tool"] == "get_kmers"]


def _chunk():
    from panfeed_amd import _lib
    return int(_lib.load().pf_gzip_device_chunk_bytes())


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


def _members(raw):
    out, at = [], 0
    for n in member_sizes(raw):
        out.append(raw[at:at + n])
        at += n
    return out


def _shape(raw, text):
    """the file's shape, for any route that made it: every member one the device decoder takes, none empty, the header
    line alone in the first; -> the text bytes of each member"""
    if not text:
        assert gzip.decompress(raw) == b"" and raw[:4] == b"\x1f\x8b\x08\x00"     # (a run without clusters: one empty member)
        return []
    ms = _members(raw)
    isize = [int.from_bytes(m[-4:], "little") for m in ms]
    assert max(len(m) for m in ms) <= slot_bytes(_chunk())
    assert max(isize) <= _chunk() and min(isize) > 0
    assert all(m[:8] == raw[:8] for m in ms) and raw[:8] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00"
    assert [len(gzip.decompress(m)) for m in ms] == isize
    assert gzip.decompress(ms[0]) == text[:text.index(b"\n") + 1]
    return isize


def _gz_run(tmp_path, argv, name="annotated.tsv.gz"):
    """the command with --gz-output: (the file's bytes, its inflated text as str); nothing goes to `out`"""
    p = tmp_path / name
    p.write_bytes(b"something older and longer than a header " * 100)          # an existing file is overwritten
    got, rc = _get_kmers(argv + ["--gz-output", str(p)])
    assert rc == 0 and got == ""
    raw = p.read_bytes()
    return raw, gzip.decompress(raw).decode()


def _same_as_reference(got, run):
    """the comparison of test_gpu_n4.py"""
    gl, el = got.splitlines(), run["stdout"].splitlines()
    assert gl[:1] == el[:1]
    assert sorted(gl[1:]) == sorted(el[1:])
    n_clusters = len({ln.split("\t")[0] for ln in el[1:]})
    cpi = int(run["args"][run["args"].index("--clusters-per-iteration") + 1]) if "--clusters-per-iteration" in run["args"] else 15
    if n_clusters <= cpi and "--only-passing" not in run["args"]:
        assert got == run["stdout"]


@pytest.mark.parametrize("host_join", [False, True], ids=["device", "host_join"])
@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{i}" for c, i in RUNS])
def test_golden_runs(tmp_path, case, i, host_join):
    from panfeed_amd.downstream import KmerJoin
    fx = next(f for f in FIX if f["case"] == case)
    run = fx["runs"][i]
    exp = CASES[case]["expect"]
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        (tmp_path / name).write_text(exp[name])
    (tmp_path / "assoc.tsv").write_text(fx["associations"])
    argv = ["-a", str(tmp_path / "assoc.tsv"), "-p", str(tmp_path / "kmers_to_hashes.tsv"), "-k", str(tmp_path / "kmers.tsv")]
    argv += run["args"] + (["--host-join"] if host_join else [])
    plain, rc = _get_kmers(argv)
    assert rc == run["rc"] == 0
    _same_as_reference(plain, run)
    before = _routes()
    raw, text = _gz_run(tmp_path, argv)
    device, host, refused = (b - a for a, b in zip(before, _routes()))
    assert text == plain
    isize = _shape(raw, text.encode())
    assert host == 0 and refused == 0 and (device > 0) == (bool(plain) and not host_join)
    if device and "--only-passing" not in run["args"]:
        st = KmerJoin.last_stats
        print(st)
        header = len(text.split("\n", 1)[0]) + 1
        assert st["gzip_text_bytes"] == len(text.encode()) - header and st["gzip_member_bytes"] == len(raw) - member_sizes(raw)[0]
        # (two of the golden cases have no target strain: kmers.tsv is its header, and the table is)
        assert (st["gzip_ms"] > 0) == (st["gzip_text_bytes"] > 0) and sum(isize[1:]) == st["gzip_text_bytes"]
    elif device:                                                               # the raw rows stayed text and went to pandas
        assert KmerJoin.last_stats["gzip_text_bytes"] == 0 == KmerJoin.last_stats["gzip_member_bytes"]


def _handmade_files(tmp_path, t):
    (tmp_path / "assoc.tsv").write_text(t["assoc"])
    (tmp_path / "kh.tsv").write_bytes(t["kh"])
    (tmp_path / "kmers.tsv").write_bytes(t["kmers"])
    return ["-a", str(tmp_path / "assoc.tsv"), "-p", str(tmp_path / "kh.tsv"), "-k", str(tmp_path / "kmers.tsv")]


def _model(tmp_path, t, per, args=()):
    return jt.join_model(str(tmp_path / "assoc.tsv"), t["kh"], t["kmers"], threshold=0.5, per_iteration=per,
                         only_passing="--only-passing" in args)


FLAGGED = {jt.TABS: ("g", "s1", "gene", "NODE_1", "1", "5", "36", "0", "31", "1"),
           jt.BYTES: ("g", "café", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.INT: ("g", "s1", "gene", "NODE_1", "1", "007", "36", "0", "31", "1", "ACG"),
           jt.EMPTY: ("g", "s1", "", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.NA: ("g", "NA", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.NUMERIC: ("g", "123", "gene", "NODE_1", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.WORD: ("g", "s1", "gene", "True", "1", "5", "36", "0", "31", "1", "ACG"),
           jt.LONG: ("g", "s1", "g" * 4096, "NODE_1", "1", "5", "36", "0", "31", "1", "ACG")}


@pytest.mark.parametrize("flag", sorted(FLAGGED), ids=[str(f) for f in sorted(FLAGGED)])
def test_a_flagged_bunch_is_host_text_in_the_same_file(tmp_path, flag):
    """the cases of test_gpu_kmerjoin.py::test_a_flagged_bunch_goes_through_pandas: the first bunch, header line and all,
    is what pandas printed, the other five are the device's members"""
    row = "\t".join(FLAGGED[flag]).encode()
    assert jt.plainness(row) == flag
    t = jt.handmade(rows_per_cluster=6)
    rows = t["kmers"].split(b"\n")
    rows.insert(3, row)
    t["kmers"] = b"\n".join(rows)
    argv = _handmade_files(tmp_path, t) + ["-t", "0.5", "--clusters-per-iteration", "1"]
    model, routes = _model(tmp_path, t, 1)
    assert routes == [False] + [True] * 5
    before = _routes()
    raw, text = _gz_run(tmp_path, argv)
    assert text == model
    assert tuple(b - a for a, b in zip(before, _routes())) == (5, 1, 0)
    _shape(raw, text.encode())


BIG = dict(rows_per_cluster=400, long_notes=300)


def _call_ends(isize, chunk):
    """the members behind the header's, split where a call's text ended: behind every member that is not full"""
    calls, cur = [], []
    for n in isize[1:]:
        cur.append(n)
        if n < chunk:
            calls.append(cur)
            cur = []
    return calls + ([cur] if cur else [])


@pytest.mark.parametrize("args", [[], ["--only-passing"]], ids=["right", "left"])
def test_handmade_table_a_bunch_a_call(tmp_path, args):
    """--clusters-per-iteration 1: six small calls, of which `full` writes more than two chunks -- one encode of at least
    three members, the last one short -- and `absent` selects no row and hands out no member"""
    from panfeed_amd.downstream import KmerJoin
    t = jt.handmade(final_newline=True, **BIG)       # (a last row without its newline is a block, and so a call, of its own)
    argv = _handmade_files(tmp_path, t) + ["-t", "0.5", "--clusters-per-iteration", "1"] + args
    model, routes = _model(tmp_path, t, 1, args)
    assert routes == [True] * 6
    rows = jt.rows_of(t["kmers"])
    per_bunch = [sum(len(r) for r in model.encode().split(b"\n") if r.split(b"\t")[0] == c) for c in (b"full", b"absent")]
    raw, text = _gz_run(tmp_path, argv)
    assert text == model
    isize = _shape(raw, text.encode())
    st = KmerJoin.last_stats
    print(st, per_bunch, isize)
    if args:
        assert st["gzip_member_bytes"] == 0 and st["raw_rows"] > 0
        return
    chunk = _chunk()
    assert per_bunch[0] > 2 * chunk and per_bunch[1] == 0 and len(rows) == 6 * BIG["rows_per_cluster"]
    calls = _call_ends(isize, chunk)
    assert len(calls) == 5                                                     # g, gx, gxy, alone, full; none for `absent`
    assert max(len(c) for c in calls) >= 3 and all(c[-1] < chunk for c in calls)
    assert st["gzip_text_bytes"] == sum(isize[1:]) and st["rows_written"] == len(model.splitlines()) - 1
    # the encoder's memory does not follow the text: slots and token streams for one slice, the members of this run's largest call
    assert st["gzip_device_bytes"] < (256 << 20)


def test_handmade_table_in_small_blocks(tmp_path):
    """kmers.tsv in blocks of 5 000 bytes: a bunch's rows come from several join calls, each call's members end with it"""
    from panfeed_amd import downstream
    t = jt.handmade(**BIG)
    argv = _handmade_files(tmp_path, t) + ["-t", "0.5", "--clusters-per-iteration", "1"]
    model, routes = _model(tmp_path, t, 1)
    old = downstream.BLOCK_BYTES
    try:
        downstream.BLOCK_BYTES = 5000
        raw, text = _gz_run(tmp_path, argv)
    finally:
        downstream.BLOCK_BYTES = old
    assert text == model and routes == [True] * 6
    isize = _shape(raw, text.encode())
    in_bunch = [sum(len(r) + 1 for r in jt.rows_of(t["kmers"]) if r.split(b"\t")[0] == c) for c in (b"g", b"gx", b"gxy", b"alone", b"full")]
    assert min(in_bunch) > 4 * 5000                   # every bunch's rows lie in five blocks or more: as many calls write rows
    assert len(_call_ends(isize, _chunk())) >= 5 * 5


# ------------------------------------------------------------------------------------------------ the library call
def _library_join(tmp_path, flags, mode=0, gz=True):
    """one bunch (`full` and `g`) of the hand-made kmers.tsv through KmerJoin itself: (what write() got, joined; the
    model's text; stats)"""
    from panfeed_amd.downstream import KmerJoin
    t = jt.handmade(final_newline=True, **BIG)       # (the whole file is one block and one join call)
    p = tmp_path / "kmers.tsv"
    p.write_bytes(t["kmers"])
    keys = [(b"full", b"CCA"), (b"full", b"CCAG"), (b"g", b"ACG")]
    text0 = [b"H5\t0.5\t" + b"n" * 40, b"H6\t1e-9\t", b"H1\t\t" + b"m" * 250]
    text1 = [x + b".0" for x in text0]
    kj = KmerJoin([(b"full", 0), (b"g", 0), (b"gx", 1)], 2, keys, text0, text1, b"\t\t")
    try:
        if gz:
            kj.set_gzip(True, flags)
        plan = kj.survey_file(str(p))
        assert plan[0]["flags"] == 0 and plan[0]["unmatched"] > 0
        got = []
        kj.join_file(str(p), 0, mode, lambda piece: got.append(bytes(piece)))
        st = kj.stats()
    finally:
        kj.close()
    rows = jt.rows_of(t["kmers"])
    if mode == 2:
        return b"".join(got), jt.kept_rows(rows, {b"full", b"g"}, set(keys)), st
    return b"".join(got), jt.join_rows(rows, {b"full", b"g"}, dict(zip(keys, text1 if mode else text0)), b"\t\t"), st


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("flag", ["0", "GZ_FIXED_ONLY", "GZ_DYNAMIC_ONLY", "GZ_LITERALS_ONLY"])
def test_encoder_flags_give_the_same_text(tmp_path, flag, mode):
    from panfeed_amd import _lib
    flags = 0 if flag == "0" else getattr(_lib, flag)
    members, model, st = _library_join(tmp_path, flags, mode)
    assert len(model) > 2 * _chunk()
    assert gzip.decompress(members) == model
    ms = _members(members)
    assert len(ms) == -(-len(model) // _chunk()) and st["gzip_text_bytes"] == len(model) and st["gzip_member_bytes"] == len(members)
    btype = {(m[10] >> 1) & 3 for m in ms}                                     # BFINAL, then BTYPE, open the payload
    assert all(m[10] & 1 for m in ms)
    if flags == _lib.GZ_FIXED_ONLY:
        assert btype == {1}
    if flags == _lib.GZ_DYNAMIC_ONLY:
        assert btype == {2}
    if flags == _lib.GZ_LITERALS_ONLY:
        plain_members, _, _ = _library_join(tmp_path, 0, mode)
        assert len(members) > len(plain_members)


def test_raw_rows_stay_text_and_the_switch_can_be_off(tmp_path):
    from panfeed_amd import _lib
    from panfeed_amd.downstream import KJ_RAW
    got, model, st = _library_join(tmp_path, 0, KJ_RAW)
    assert got == model and model and st["gzip_text_bytes"] == 0
    got, model, st = _library_join(tmp_path, 0, 0, gz=False)
    assert got == model and st["gzip_member_bytes"] == 0
    with pytest.raises(_lib.PanfeedHipError) as ei:
        _library_join(tmp_path, 8)
    assert ei.value.status == _lib.ERR_ARG


def test_a_run_without_clusters(tmp_path):
    """no hash passes: nothing is printed without the option, and the file is a valid gzip file of no text"""
    t = jt.handmade(rows_per_cluster=6)
    argv = _handmade_files(tmp_path, t) + ["-t", "1e-30"]
    plain, rc = _get_kmers(argv)
    raw, text = _gz_run(tmp_path, argv)
    assert rc == 0 and plain == "" == text
    _shape(raw, b"")
