"""--passing-hashes / --passing-associations of the `panfeed` command (panfeed_amd/cli.py) without a GPU: the refusals
and their status, the digest file's parsing, the mapping onto run_files' `passing_hashes`.  The work is a recording
stand-in for run_files, the associations reader one for downstream._associations (tests/test_gpu_passing_rows.py runs the
real ones)."""
import base64
import logging
import os

import pytest

from panfeed_amd import cli

BASE = ["-g", "gffs", "-p", "table.csv"]
H1 = base64.b64encode(bytes(range(16))).decode()
H2 = base64.b64encode(bytes(range(16, 32))).decode()
TODAY = dict(fastadir=None, klength=31, canon=True, consider_missing=False, patfilt=True, maf=0.01, upstream=0,
             downstream=0, downstream_start_codon=False, targets=(), genes=None, compress=False,
             multiple_files=False, batch_clusters=256, device=0, raise_missing=False)


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *a, **kw):
        self.calls.append((a, kw))
        return {"clusters": 0, "instances": 0, "patterns": 0, "log": "", "kmers_rows_considered": 7, "kmers_rows_kept": 3}


def _run(tmp_path, argv, **kw):
    rec = Recorder()
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        rc = cli.main(argv, run=rec, **kw)
    finally:
        os.chdir(old)
    return rc, rec


def _never(*a, **kw):
    raise AssertionError("nothing may be started")


@pytest.mark.parametrize("extra", [
    ["--passing-hashes", "no_such.txt", "--passing-associations", "no_such.tsv"],
    ["--passing-threshold", "0.05"],
    ["--passing-column", "pvalue"],
    ["--passing-hashes", "no_such.txt", "--passing-threshold", "0.05"],
    ["--passing-hashes", "no_such.txt", "--passing-column", "pvalue"],
    ["--passing-hashes", "no_such.txt", "--gpus", "2"],
    ["--passing-associations", "no_such.tsv", "--gpus", "2"],
])
def test_refusals_with_status_2_before_any_file_is_read(tmp_path, extra):
    rc, rec = _run(tmp_path, BASE + ["--targets", "no_such_file.txt"] + extra, launch=_never, rank_entry=_never,
                   associations=_never)
    assert rc == 2 and not rec.calls
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra", [["--passing-hashes", "no_such.txt"], ["--passing-associations", "no_such.tsv"]])
def test_a_launched_rank_is_refused_and_says_so(tmp_path, monkeypatch, caplog, extra):
    caplog.set_level(logging.ERROR, logger="panfeed")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    rc, rec = _run(tmp_path, BASE + extra, launch=_never, rank_entry=_never, associations=_never)
    assert rc == 2 and not rec.calls
    assert any("launched rank" in r.getMessage() and "scope" in r.getMessage() for r in caplog.records)


def test_gpus_refusal_says_so(tmp_path, caplog):
    caplog.set_level(logging.ERROR, logger="panfeed")
    rc, rec = _run(tmp_path, BASE + ["--passing-hashes", "no_such.txt", "--gpus", "2"], launch=_never)
    assert rc == 2 and any("--gpus N" in r.getMessage() for r in caplog.records)


def test_the_digest_files_lines(tmp_path, caplog):
    caplog.set_level(logging.WARNING, logger="panfeed")
    (tmp_path / "t.txt").write_text("s1\n")
    # a header word, blank lines, a 23-character line, a repeat, 24 characters that are no canonical base64 of 16 bytes
    (tmp_path / "h.txt").write_text(f"hashed_pattern\n{H1}\n\n   \n{H2[:23]}\n{H2}\r\n{H1}\n{'A' * 23}B\n")
    rc, rec = _run(tmp_path, BASE + ["--targets", "t.txt", "--passing-hashes", "h.txt"])
    assert rc == 0 and len(rec.calls) == 1
    kw = rec.calls[0][1]
    assert kw.pop("passing_hashes") == [H1, H2]
    assert kw == dict(TODAY, targets=("s1",))
    warned = [r.getMessage() for r in caplog.records if "hashed_pattern" in r.getMessage()]
    assert len(warned) == 1 and warned[0].startswith("3 entries of h.txt")


def test_an_empty_list_is_on_and_no_targets_is_accepted(tmp_path, caplog):
    caplog.set_level(logging.INFO, logger="panfeed")
    (tmp_path / "h.txt").write_text("\n")
    rc, rec = _run(tmp_path, BASE + ["--passing-hashes", "h.txt"])
    assert rc == 0 and rec.calls[0][1]["passing_hashes"] == []
    assert any("No target strains: the passing patterns" in r.getMessage() for r in caplog.records)
    assert any("3 of 7 kmers.tsv rows kept" in r.getMessage() for r in caplog.records)


def test_associations_reach_run_with_defaults_and_given_values(tmp_path):
    seen = []

    def assoc(path, threshold, column, device):
        seen.append((path, threshold, column, device))
        return [H2, "not a digest", H1]

    rc, rec = _run(tmp_path, BASE + ["--passing-associations", "a.tsv"], associations=assoc)
    assert rc == 0 and seen == [("a.tsv", 1, "lrt-pvalue", 0)]
    assert rec.calls[0][1]["passing_hashes"] == [H2, H1]
    rc, rec = _run(tmp_path, BASE + ["--passing-associations", "a.tsv", "--passing-threshold", "0.05", "--passing-column",
                                     "pvalue", "--device", "2"], associations=assoc)
    assert rc == 0 and seen[1] == ("a.tsv", 0.05, "pvalue", 2)


def test_a_missing_column_exits_1(tmp_path):
    def assoc(path, threshold, column, device):
        raise SystemExit(1)          # downstream._missing_column, after its message

    rc, rec = _run(tmp_path, BASE + ["--passing-associations", "a.tsv"], associations=assoc)
    assert rc == 1 and not rec.calls


def test_without_the_options_run_gets_todays_keywords(tmp_path):
    rc, rec = _run(tmp_path, BASE)
    assert rc == 0 and rec.calls[0][1] == TODAY


def test_python_side_digest_parsing():
    from panfeed_amd.engine import filter_passing_rows, passing_digests
    assert passing_digests([H2, bytes(range(16)), H1]) == [bytes(range(16)), bytes(range(16, 32))]
    assert passing_digests([]) == []
    for bad in (H1[:23], "A" * 23 + "B", b"short", 5):
        with pytest.raises(ValueError):
            passing_digests([bad])
    kh = f"c1\t\t{H2}\nc1\tACG\t{H1}\nc1\tCCC\t{H2}\nc2\tACG\t{H2}\n"
    kt = "c1\ts\tf\tx\t1\t0\t3\t0\t3\t1\tACG\nc2\ts\tf\tx\t1\t0\t3\t0\t3\t1\tACG\nc1\ts\tf\tx\t1\t1\t4\t1\t4\t1\tTTT\n"
    assert filter_passing_rows(kt, kh, {H1}) == (kt.split("\n")[0] + "\n", 3, 1)
