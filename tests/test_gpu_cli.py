"""`python -m panfeed_amd` (the panfeed command) against the reference's own command: every case of
tests/golden/cli.json.gz (tools/gen_golden_cli.py) replayed in a fresh process -- exit status and every output file,
byte for byte (gzip members decompressed) -- and the README's two-pass chain through the command and
panfeed_amd.downstream's get_clusters / get_kmers."""
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

GOLDEN = json.load(gzip.open(os.path.join(REPO, "tests", "golden", "cli.json.gz"), "rt"))
CASES = GOLDEN["cases"]


def materialise(files, root):
    for rel, text in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w", newline="") as fh:
            fh.write(text)


def read_outputs(out):
    if not os.path.isdir(out):
        return None
    files = {}
    for d, _sub, names in os.walk(out):
        for n in sorted(names):
            p = os.path.join(d, n)
            with (gzip.open(p, "rt", newline="") if n.endswith(".gz") else open(p, newline="")) as fh:
                files[os.path.relpath(p, out)] = fh.read()
    return files


def panfeed(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "panfeed_amd"] + args, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=600)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_equals_reference(tmp_path, case):
    materialise(GOLDEN["pangenomes"][case["pangenome"]], str(tmp_path))
    if case["pre_existing_output"]:
        os.makedirs(tmp_path / "out")
        (tmp_path / "out" / "keep.txt").write_text("untouched\n")
    p = panfeed(case["args"] + ["-o", "out", "--cores", "1"], str(tmp_path))
    exp = case["expect"]
    assert p.returncode == exp["rc"], p.stderr[-3000:]
    got = read_outputs(str(tmp_path / "out"))
    if exp["rc"] == 0:
        assert sorted(got) == sorted(exp["outputs"])
        for name, text in exp["outputs"].items():
            assert got[name] == text, name
        if "--compress" in case["args"]:
            assert all(n.endswith(".gz") for n in got)
    elif case["pre_existing_output"]:
        assert got == {"keep.txt": "untouched\n"}
    elif exp["outputs"] is None:
        assert got is None            # refused before anything was made
    if "--stop-on-missing" in case["args"]:
        assert "Could not find" in p.stderr or "Missing" in p.stderr


def _downstream(tool, argv, cwd):
    from panfeed_amd import downstream
    out = io.StringIO()
    old = os.getcwd()
    os.chdir(cwd)
    try:
        rc = (downstream.get_clusters if tool == "get_clusters" else downstream.get_kmers)(argv, out=out)
    finally:
        os.chdir(old)
    return rc, out.getvalue()


def test_two_pass_chain(tmp_path):
    ch = GOLDEN["chain"]
    root = str(tmp_path)
    materialise(GOLDEN["pangenomes"][ch["pangenome"]], root)
    p = panfeed(ch["pass1_args"] + ["-o", "pass1"], root)
    assert p.returncode == 0, p.stderr[-3000:]
    assert read_outputs(os.path.join(root, "pass1")) == ch["pass1"]
    with open(os.path.join(root, "assoc.tsv"), "w") as fh:
        fh.write(ch["associations"])
    rc, clusters = _downstream("get_clusters", ch["clusters_args"], root)
    assert rc == 0 and sorted(clusters.splitlines()) == sorted(ch["clusters_stdout"].splitlines())
    with open(os.path.join(root, "gene_clusters.txt"), "w") as fh:
        fh.write(clusters)
    p = panfeed(ch["pass2_args"] + ["-o", "pass2"], root)
    assert p.returncode == 0, p.stderr[-3000:]
    assert read_outputs(os.path.join(root, "pass2")) == ch["pass2"]
    rc, kmers = _downstream("get_kmers", ch["kmers_args"], root)
    assert rc == 0
    gl, el = kmers.splitlines(), ch["kmers_stdout"].splitlines()
    assert gl[:1] == el[:1] and sorted(gl[1:]) == sorted(el[1:])
