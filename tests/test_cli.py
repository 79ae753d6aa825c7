"""The `panfeed` command (`python -m panfeed_amd`, panfeed_amd/cli.py) without a GPU: argument handling, the refusals
and their exit statuses, the mapping onto pipeline.run_files' arguments, the --targets / --genes files.  The work itself
is a recording stand-in for run_files (tests/test_gpu_cli.py runs the real thing)."""
import os
import subprocess
import sys

import pytest

from conftest import REPO
from panfeed_amd import __version__, cli


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *a, **kw):
        self.calls.append((a, kw))
        return {"clusters": 0, "instances": 0, "patterns": 0, "log": ""}


def _run(tmp_path, argv, **kw):
    rec = Recorder()
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        rc = cli.main(argv, run=rec, **kw)
    finally:
        os.chdir(old)
    return rc, rec


BASE = ["-g", "gffs", "-p", "table.csv"]


def test_defaults_map_onto_run_files(tmp_path):
    rc, rec = _run(tmp_path, BASE)
    assert rc == 0 and len(rec.calls) == 1
    a, kw = rec.calls[0]
    assert a == ("table.csv", "gffs", "panfeed")
    assert kw == dict(fastadir=None, klength=31, canon=True, consider_missing=False, patfilt=True, maf=0.01, upstream=0,
                      downstream=0, downstream_start_codon=False, targets=(), genes=None, compress=False,
                      multiple_files=False, batch_clusters=256, device=0, raise_missing=False)


def test_flags_map_onto_run_files(tmp_path):
    rc, rec = _run(tmp_path, BASE + ["-o", "out", "-f", "fas", "-k", "21", "--maf", "0.2", "--upstream", "100",
                                     "--downstream", "50", "--downstream-start-codon", "--non-canonical", "--no-filter",
                                     "--consider-missing", "--multiple-files", "--compress", "--stop-on-missing",
                                     "--device", "3", "--batch-clusters", "17", "--cores", "8", "-ql", "5", "-vv"])
    assert rc == 0
    a, kw = rec.calls[0]
    assert a == ("table.csv", "gffs", "out")
    assert kw == dict(fastadir="fas", klength=21, canon=False, consider_missing=True, patfilt=False, maf=0.2,
                      upstream=100, downstream=50, downstream_start_codon=True, targets=(), genes=None, compress=True,
                      multiple_files=True, batch_clusters=17, device=3, raise_missing=True)


def test_long_option_spellings(tmp_path):
    rc, rec = _run(tmp_path, ["--gff", "g", "--presence-absence", "t.csv", "--output", "o", "--fasta", "f",
                              "--kmer-length", "19", "--queue-limit", "2"])
    assert rc == 0
    a, kw = rec.calls[0]
    assert a == ("t.csv", "g", "o") and kw["fastadir"] == "f" and kw["klength"] == 19


def test_targets_and_genes_files(tmp_path):
    # one name per line, only the trailing newline stripped: blanks stay part of a name; the file is read in text mode,
    # as the reference reads it, so '\r\n' ends a line too (input.py:198-211)
    (tmp_path / "t.txt").write_text("s2\ns1\n s3\ns1\nlast")
    (tmp_path / "g.txt").write_text("grp_b\ngrp_a\r\n\n")
    rc, rec = _run(tmp_path, BASE + ["--targets", "t.txt", "--genes", "g.txt"])
    assert rc == 0
    kw = rec.calls[0][1]
    assert kw["targets"] == (" s3", "last", "s1", "s2")
    assert kw["genes"] == ["", "grp_a", "grp_b"]


def test_no_targets_warns(tmp_path, caplog):
    import logging
    caplog.set_level(logging.WARNING, logger="panfeed")
    rc, rec = _run(tmp_path, BASE)
    assert rc == 0 and rec.calls[0][1]["targets"] == ()
    assert any("target" in r.getMessage().lower() for r in caplog.records)


@pytest.mark.parametrize("extra,status", [
    (["--downstream-start-codon", "--upstream", "10", "--downstream", "20"], 1),       # 30 < k = 31
    (["--downstream-start-codon", "-k", "15", "--upstream", "7", "--downstream", "7"], 1),
    (["--maf", "0.51"], 1),
    (["-k", "127"], 2),
    (["-k", "0"], 2),
])
def test_refusals_before_any_file_is_read(tmp_path, extra, status):
    """the two checks of the reference and the k range: nothing is read (the inputs do not exist), nothing created"""
    rc, rec = _run(tmp_path, BASE + ["--targets", "no_such_file.txt"] + extra)
    assert rc == status and not rec.calls
    assert os.listdir(tmp_path) == []


def test_start_codon_check_passes_at_k(tmp_path):
    rc, rec = _run(tmp_path, BASE + ["--downstream-start-codon", "-k", "15", "--upstream", "7", "--downstream", "8"])
    assert rc == 0 and len(rec.calls) == 1


def test_k_limit_names_pf_max_k(tmp_path, caplog):
    import logging
    caplog.set_level(logging.ERROR, logger="panfeed")
    rc, _ = _run(tmp_path, BASE + ["-k", "200"])
    assert rc != 0
    assert any("PF_MAX_K" in r.getMessage() and "126" in r.getMessage() for r in caplog.records)
    with open(os.path.join(REPO, "include", "panfeed_hip.h")) as fh:
        assert f"#define PF_MAX_K {cli.PF_MAX_K} " in fh.read()


def test_existing_output_is_refused_and_left_alone(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    (out / "keep.txt").write_text("untouched\n")
    rc, rec = _run(tmp_path, BASE + ["-o", "out"])
    assert rc == 1 and not rec.calls
    assert os.listdir(out) == ["keep.txt"] and (out / "keep.txt").read_text() == "untouched\n"


def test_stop_on_missing_error_exits_non_zero(tmp_path, caplog):
    import logging
    from panfeed_amd._lib import PanfeedHipError

    def failing(*a, **kw):
        assert kw["raise_missing"]
        raise PanfeedHipError(-1, "Could not find gene g7 from grp_x in s3")
    caplog.set_level(logging.ERROR, logger="panfeed")
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        rc = cli.main(BASE + ["--stop-on-missing"], run=failing)
    finally:
        os.chdir(old)
    assert rc != 0
    assert any("Could not find gene g7 from grp_x in s3" in r.getMessage() for r in caplog.records)


def test_reader_warnings_are_logged(tmp_path, caplog):
    import logging
    caplog.set_level(logging.WARNING, logger="panfeed")
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        rc = cli.main(BASE, run=lambda *a, **kw: {"log": "Could not find gene x from y in z\n"})
    finally:
        os.chdir(old)
    assert rc == 0 and any("Could not find gene x" in r.getMessage() for r in caplog.records)


def _module(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "panfeed_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=120)


def test_module_version_and_help(tmp_path):
    p = _module(["--version"], tmp_path)
    assert p.returncode == 0 and p.stdout.strip() == f"panfeed {__version__}"
    p = _module(["--help"], tmp_path)
    assert p.returncode == 0
    for opt in ("--gff", "--presence-absence", "--targets", "--genes", "--output", "--fasta", "--maf", "--upstream",
                "--downstream", "--downstream-start-codon", "--non-canonical", "--no-filter", "--consider-missing",
                "--multiple-files", "--compress", "--cores", "--queue-limit", "--stop-on-missing", "--device",
                "--batch-clusters", "--version", "-ql", "-k"):
        assert opt in p.stdout, opt
    assert "torchrun" in p.stdout


def test_module_refusals_without_a_gpu(tmp_path):
    """in a fresh process, the refusals exit with their status before the library is loaded"""
    p = _module(["-g", "gffs", "-p", "t.csv", "--maf", "0.9"], tmp_path)
    assert p.returncode == 1 and "maf" in p.stderr
    p = _module(["-g", "gffs", "-p", "t.csv", "-k", "130"], tmp_path)
    assert p.returncode != 0 and "PF_MAX_K" in p.stderr
    (tmp_path / "panfeed").mkdir()
    p = _module(["-g", "gffs", "-p", "t.csv"], tmp_path)
    assert p.returncode == 1 and os.listdir(tmp_path / "panfeed") == []
    assert p.returncode == 1 and sorted(os.listdir(tmp_path)) == ["panfeed"]
    p = _module(["-p", "t.csv"], tmp_path)
    assert p.returncode == 2                   # argparse: -g is required
