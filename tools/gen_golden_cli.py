#!/usr/bin/env python3
"""Generate tests/golden/cli.json.gz: the REFERENCE's own `panfeed` command (`panfeed/__main__.py:main`, `--cores 1`)
run in this container over small seeded pangenomes written by `synth.write_pangenome`, for the option matrix of the
`python -m panfeed_amd` command (tests/test_gpu_cli.py replays every case).

pyfaidx is bound to the declared double of tools/gen_golden_n1.py (imported from there, not restated).

Stored per case: the input files we made (texts), the arguments, the exit status and every output file's text (gzip
members decompressed; the empty `<output>/fastas/` directory the reference leaves behind is not an output).  Also one
two-pass chain (the README's workflow): pass 1 -> a made-up association table over pass 1's hashes -> the reference's
`get_clusters.main` -> pass 2 (every strain a target, `--genes` = that list) -> `get_kmers.main`, each stage's output
kept.  Data only: no text of the reference.

Usage: python tools/gen_golden_cli.py            (rewrites tests/golden/cli.json.gz; build container only)
"""
import contextlib
import gzip
import io
import json
import logging
import os
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_golden_n1  # noqa: E402,F401  (binds pyfaidx to its declared double, puts the reference on sys.path)
from gen_golden_n1 import synth_pangenome  # noqa: E402
from gen_golden_n4 import associations  # noqa: E402

from panfeed import __main__ as ref_main  # noqa: E402  (reference)
from panfeed import get_clusters as ref_get_clusters  # noqa: E402
from panfeed import get_kmers as ref_get_kmers  # noqa: E402


def materialise(files, root):
    for rel, text in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w", newline="") as fh:
            fh.write(text)


def read_outputs(out):
    """{relative path: text} of every file under `out` (.gz decompressed, the name kept); None when there is no `out`"""
    if not os.path.isdir(out):
        return None
    files = {}
    for d, _sub, names in os.walk(out):
        for n in sorted(names):
            p = os.path.join(d, n)
            rel = os.path.relpath(p, out)
            with (gzip.open(p, "rt", newline="") if n.endswith(".gz") else open(p, newline="")) as fh:
                files[rel] = fh.read()
    return files


def run_main(main, argv, cwd):
    """main() of a reference tool with sys.argv = argv, in `cwd`: (exit status, stdout)"""
    old_argv, old_cwd = sys.argv, os.getcwd()
    sys.argv = argv
    os.chdir(cwd)
    buf = io.StringIO()
    rc = 0
    try:
        with contextlib.redirect_stdout(buf):
            try:
                main()
            except SystemExit as e:
                rc = int(e.code or 0) if not isinstance(e.code, str) else 1
            except Exception:               # noqa: BLE001  (an uncaught exception: Python exits with 1)
                rc = 1
    finally:
        sys.argv = old_argv
        os.chdir(old_cwd)
        logging.getLogger("panfeed").handlers.clear()
    return rc, buf.getvalue()


def run_case(files, args, pre_existing_output=False):
    root = tempfile.mkdtemp(prefix="golden_cli_")
    try:
        materialise(files, root)
        if pre_existing_output:
            os.makedirs(os.path.join(root, "out"))
            with open(os.path.join(root, "out", "keep.txt"), "w") as fh:
                fh.write("untouched\n")
        rc, _ = run_main(ref_main.main, ["panfeed"] + args + ["-o", "out", "--cores", "1"], root)
        outs = read_outputs(os.path.join(root, "out"))
        return {"rc": rc, "outputs": outs}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def file_of_files(files, prefix, exts):
    """the text of a file naming every input file under `prefix` with one of `exts`, one relative path per line"""
    return "".join(p + "\n" for p in sorted(files) if p.startswith(prefix) and p.endswith(exts))


def main():
    pangenomes, cases = {}, []

    # A: GFFs with their ##FASTA sections, one strain without a GFF, 'N's, paralogs
    files, names_a = synth_pangenome(21, 10, 7, flank=0, mean_len=140, min_len=40, max_len=400, n_rate=0.02,
                                     paralog_rate=0.1, drop=(3,), wrap=60, missing_gene_rate=0.0)
    files["gffs.txt"] = file_of_files(files, "gffs/", (".gff",))
    files["targets.txt"] = names_a[0] + "\n" + names_a[5] + "\n"
    files["all_targets.txt"] = "".join(n + "\n" for n in names_a)
    table = [ln.split(",")[0] for ln in files["gene_presence_absence.csv"].split("\n")[1:] if ln]
    files["genes.txt"] = table[1] + "\n" + table[6] + "\n" + "not_a_cluster\n"
    pangenomes["a"] = files
    # B: some strains' sequences in separate FASTA files
    files, names_b = synth_pangenome(22, 8, 6, flank=10, mean_len=120, min_len=30, max_len=300, n_rate=0.03,
                                     paralog_rate=0.05, sep=(1, 4), wrap=50, missing_gene_rate=0.0)
    files["gffs.txt"] = file_of_files(files, "gffs/", (".gff",))
    files["fastas.txt"] = file_of_files(files, "gffs/", (".fasta", ".fna"))
    files["targets.txt"] = names_b[1] + "\n" + names_b[2] + "\n"
    pangenomes["b"] = files
    # C: a gene the table names but no GFF holds (--stop-on-missing)
    files, _ = synth_pangenome(23, 5, 5, flank=0, mean_len=100, min_len=40, max_len=200, n_rate=0.0, paralog_rate=0.0,
                               wrap=60, missing_gene_rate=0.3)
    pangenomes["c"] = files

    def add(name, pg, args, **kw):
        cases.append({"name": name, "pangenome": pg, "args": args, "pre_existing_output": kw.get("pre", False),
                      "expect": run_case(pangenomes[pg], args, kw.get("pre", False))})

    base = ["-g", "gffs", "-p", "gene_presence_absence.csv", "-k", "15"]
    add("plain", "a", base)
    add("compress", "a", base + ["--compress"])
    add("multiple_files", "a", base + ["--multiple-files"])
    add("targets", "a", base + ["--targets", "targets.txt"])
    add("genes", "a", base + ["--genes", "genes.txt", "--targets", "targets.txt"])
    add("consider_missing", "a", base + ["--consider-missing"])
    add("non_canonical", "a", base + ["--non-canonical", "--targets", "targets.txt"])
    add("no_filter", "a", base + ["--no-filter"])
    add("maf_0.2", "a", base + ["--maf", "0.2"])
    add("flanks", "a", base + ["--upstream", "30", "--downstream", "20", "--targets", "targets.txt"])
    add("flanks_start_codon", "a", base + ["--upstream", "10", "--downstream", "40", "--downstream-start-codon"])
    add("k31_defaults", "a", ["-g", "gffs", "-p", "gene_presence_absence.csv", "--targets", "all_targets.txt"])
    add("gff_file_of_files", "a", ["-g", "gffs.txt", "-p", "gene_presence_absence.csv", "-k", "21"])
    add("fasta_dir", "b", ["-g", "gffs", "-f", "gffs", "-p", "gene_presence_absence.csv", "-k", "17",
                           "--targets", "targets.txt"])
    add("fasta_file_of_files", "b", ["-g", "gffs.txt", "-f", "fastas.txt", "-p", "gene_presence_absence.csv", "-k", "17",
                                     "--compress"])
    add("consider_missing_all_gffs", "b", ["-g", "gffs", "-f", "gffs", "-p", "gene_presence_absence.csv", "-k", "13",
                                           "--consider-missing", "--targets", "targets.txt"])
    add("missing_gene_warns", "c", ["-g", "gffs", "-p", "gene_presence_absence.csv", "-k", "11"])
    # refusals
    add("refuse_start_codon_short", "a", base + ["--upstream", "5", "--downstream", "5", "--downstream-start-codon"])
    add("refuse_maf", "a", base + ["--maf", "0.6"])
    add("refuse_existing_output", "a", base, pre=True)
    add("refuse_stop_on_missing", "c", ["-g", "gffs", "-p", "gene_presence_absence.csv", "-k", "11", "--stop-on-missing"])

    # the two-pass chain over pangenome A
    chain = {"pangenome": "a", "pass1_args": base + ["--upstream", "20", "--downstream", "20"]}
    root = tempfile.mkdtemp(prefix="golden_cli_chain_")
    try:
        materialise(pangenomes["a"], root)
        rc, _ = run_main(ref_main.main, ["panfeed"] + chain["pass1_args"] + ["-o", "pass1", "--cores", "1"], root)
        assert rc == 0
        chain["pass1"] = read_outputs(os.path.join(root, "pass1"))
        chain["associations"] = associations(chain["pass1"]["kmers_to_hashes.tsv"], 31, nan_rate=0.0)
        with open(os.path.join(root, "assoc.tsv"), "w") as fh:
            fh.write(chain["associations"])
        chain["clusters_args"] = ["-a", "assoc.tsv", "-p", "pass1/kmers_to_hashes.tsv", "-t", "0.05"]
        rc, out = run_main(ref_get_clusters.main, ["panfeed-get-clusters"] + chain["clusters_args"], root)
        assert rc == 0
        chain["clusters_stdout"] = out
        with open(os.path.join(root, "gene_clusters.txt"), "w") as fh:
            fh.write(out)
        chain["pass2_args"] = base + ["--upstream", "20", "--downstream", "20", "--targets", "all_targets.txt",
                                      "--genes", "gene_clusters.txt"]
        rc, _ = run_main(ref_main.main, ["panfeed"] + chain["pass2_args"] + ["-o", "pass2", "--cores", "1"], root)
        assert rc == 0
        chain["pass2"] = read_outputs(os.path.join(root, "pass2"))
        chain["kmers_args"] = ["-a", "assoc.tsv", "-p", "pass2/kmers_to_hashes.tsv", "-k", "pass2/kmers.tsv", "-t", "0.05"]
        rc, out = run_main(ref_get_kmers.main, ["panfeed-get-kmers"] + chain["kmers_args"], root)
        assert rc == 0
        chain["kmers_stdout"] = out
    finally:
        shutil.rmtree(root, ignore_errors=True)

    out = os.path.join(REPO, "tests", "golden", "cli.json.gz")
    payload = json.dumps({"pangenomes": pangenomes, "cases": cases, "chain": chain}, sort_keys=True,
                         separators=(",", ":")).encode()
    with open(out, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as fh:
            fh.write(payload)
    print(f"{out}: {len(cases)} cases over {len(pangenomes)} pangenomes, exit statuses "
          f"{[c['expect']['rc'] for c in cases]}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
