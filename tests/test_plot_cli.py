"""panfeed-plot's command line (panfeed_amd/plot.py), no GPU: options and defaults as the reference's, the refusals with
their status and order, and that `--help` and the refusals never load libpanfeed_hip.so."""
import gzip
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO

with gzip.open(os.path.join(GOLDEN, "plot.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
SYN = next(f for f in FIX if f["name"] == "synthetic")


def test_defaults_are_the_references():
    from panfeed_amd.plot import get_options
    a = get_options(["-k", "k.tsv", "-p", "p.tsv"])
    assert (a.column, a.threshold, a.phenotype_column, a.sample, a.start, a.stop) == ("lrt-pvalue", 1, None, None, None, None)
    assert (a.format, a.output_directory, a.dpi, a.minimum_pvalue, a.nucleotides) == ("png", ".", 300, 1e-10, False)
    assert (a.alpha, a.xticks, a.height, a.width, a.v, a.device) == (0, 200, 9.0, 10.0, 0, 0)
    b = get_options(["--kmers", "k", "--phenotype", "p", "-c", "x", "-t", "0.5", "--start", "-3", "--stop", "4",
                     "--format", "svg", "--nucleotides", "-v", "-v", "--device", "1"])
    assert (b.column, b.threshold, b.start, b.stop, b.format, b.nucleotides, b.v, b.device) == \
        ("x", 0.5, -3, 4, "svg", True, 2, 1)


@pytest.mark.parametrize("argv", [[], ["-k", "x"], ["-p", "y"], ["-k", "x", "-p", "y", "--format", "jpg"]])
def test_bad_command_lines_exit_2(argv):
    from panfeed_amd.plot import plot
    with pytest.raises(SystemExit) as e:
        plot(argv)
    assert e.value.code == 2


def _files(tmp_path):
    pk, pp = tmp_path / "k.tsv", tmp_path / "p.tsv"
    pk.write_text(SYN["kmers"])
    pp.write_text(SYN["phenotype"])
    return str(pk), str(pp)


@pytest.mark.parametrize("i", [i for i, r in enumerate(SYN["runs"]) if r["rc"] != 0])
def test_refusals_as_the_reference(tmp_path, i):
    from panfeed_amd.plot import plot
    run = SYN["runs"][i]
    pk, pp = _files(tmp_path)
    assert plot(["-k", pk, "-p", pp, "--output-directory", str(tmp_path)] + run["args"]) == run["rc"]
    assert [f for f in os.listdir(tmp_path) if f.endswith(".png")] == []


def test_refusal_order(tmp_path, caplog):
    """options first (sample, alpha, start/stop, start > stop), then the phenotype column, then the p-value column"""
    from panfeed_amd.plot import plot
    pk, pp = _files(tmp_path)
    cases = [
        (["--sample", "2", "--alpha", "3", "--start", "1"], "--sample should be between 0 and 1"),
        (["--alpha", "3", "--start", "1"], "--alpha should be between 0 and 1"),
        (["--stop", "1", "--phenotype-column", "nope"], "both --start and --stop are needed"),
        (["--start", "2", "--stop", "1", "-c", "nope"], "--start should be lower than --stop"),
        (["--phenotype-column", "nope", "-c", "nope"], "phenotype file does not have the nope column"),
        (["-c", "nope"], "k-mer file does not have the nope column"),
    ]
    for extra, msg in cases:
        caplog.clear()
        assert plot(["-k", pk, "-p", pp] + extra) == 1
        assert msg in [r.getMessage() for r in caplog.records if r.levelname == "WARNING"]


def test_option_refusals_read_no_file(tmp_path):
    from panfeed_amd.plot import plot
    assert plot(["-k", str(tmp_path / "none.tsv"), "-p", str(tmp_path / "none.tsv"), "--alpha", "2"]) == 1


def _fresh(code):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    return subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)


def test_help_and_refusals_in_a_fresh_process_load_no_library(tmp_path):
    pk, pp = _files(tmp_path)
    r = subprocess.run([sys.executable, "-m", "panfeed_amd.plot", "--help"], cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--phenotype-column" in r.stdout and "--device" in r.stdout
    code = ("from panfeed_amd.plot import plot\n"
            f"rcs = [plot(['-k', {pk!r}, '-p', {pp!r}, '-c', 'nope']), plot(['-k', {pk!r}, '-p', {pp!r}, '--sample', '3']),\n"
            f"       plot(['-k', {pk!r}, '-p', {pp!r}, '--phenotype-column', 'nope'])]\n"
            "maps = open('/proc/self/maps').read()\n"
            "print(rcs, 'libpanfeed_hip' in maps)\n")
    r = _fresh(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "[1, 1, 1] False"
