"""panfeed-get-clusters / panfeed-get-kmers over the files of golden cases, against the outputs of
the reference's own `main()`s (tests/golden/n4.json.gz, made by tools/gen_golden_n4.py).  The row filter runs on the
GPU (pf_rowfilter_scan).

The reference iterates over Python sets of cluster names: the order of its printed clusters (get_clusters) and of its
per-bunch blocks (get_kmers with more clusters than --clusters-per-iteration) is arbitrary, so those are compared as
multisets of lines; everything else byte for byte."""
import gzip
import io
import json
import os

import pytest

from conftest import GOLDEN, all_cases

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}
RUNS = [(f["case"], i) for f in FIX for i in range(len(f["runs"]))]


def _files(tmp_path, fx, gz=False):
    exp = CASES[fx["case"]]["expect"]
    paths = {}
    for name in ("kmers.tsv", "kmers_to_hashes.tsv"):
        p = tmp_path / (name + (".gz" if gz else ""))
        if gz:
            from panfeed_amd.output import ParallelGzipWriter
            w = ParallelGzipWriter(str(p), chunk_bytes=65536)     # several members
            w.write(exp[name])
            w.close()
        else:
            p.write_text(exp[name])
        paths[name] = str(p)
    pa = tmp_path / "assoc.tsv"
    pa.write_text(fx["associations"])
    return paths, str(pa)


def _run(tool, argv):
    from panfeed_amd import downstream
    out = io.StringIO()
    rc = 0
    try:
        rc = (downstream.get_clusters if tool == "get_clusters" else downstream.get_kmers)(argv, out=out)
    except SystemExit as e:
        rc = int(e.code or 0)
    return out.getvalue(), rc


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{i}" for c, i in RUNS])
def test_downstream_tools_equal_reference(tmp_path, case, i):
    fx = next(f for f in FIX if f["case"] == case)
    run = fx["runs"][i]
    paths, pa = _files(tmp_path, fx)
    po = str(tmp_path / "filtered.tsv")
    argv = ["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-o", po] + run["args"]
    if run["tool"] == "get_kmers":
        argv += ["-k", paths["kmers.tsv"]]
    got, rc = _run(run["tool"], argv)
    assert rc == run["rc"]
    if run["filtered"] is None:
        assert not os.path.exists(po)
    else:
        assert open(po).read() == run["filtered"]
    exp = run["stdout"]
    if run["tool"] == "get_clusters":
        assert sorted(got.splitlines()) == sorted(exp.splitlines())
        return
    gl, el = got.splitlines(), exp.splitlines()
    assert gl[:1] == el[:1]                                    # the header, once
    assert sorted(gl[1:]) == sorted(el[1:])
    n_clusters = len({ln.split("\t")[0] for ln in el[1:]})
    cpi = int(run["args"][run["args"].index("--clusters-per-iteration") + 1]) if "--clusters-per-iteration" in run["args"] else 15
    if n_clusters <= cpi and "--only-passing" not in run["args"]:
        assert got == exp                                      # one bunch: kmers.tsv order, byte for byte


def test_gzip_inputs_and_blocks(tmp_path):
    """.gz inputs (several gzip members) and blocks far smaller than the file: lines cut by block ends are carried over"""
    from panfeed_amd import downstream
    fx = FIX[0]
    paths, pa = _files(tmp_path, fx, gz=True)
    run = next(r for r in fx["runs"] if r["tool"] == "get_kmers" and r["args"] == ["-t", "0.01"])
    old = downstream.BLOCK_BYTES
    try:
        for blk in (257, 4096, old):
            downstream.BLOCK_BYTES = blk
            got, rc = _run("get_kmers", ["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-k", paths["kmers.tsv"], "-t", "0.01"])
            assert rc == 0 and got == run["stdout"], blk
    finally:
        downstream.BLOCK_BYTES = old


def test_rowfilter_exact_keys(tmp_path):
    """first-field and last-field keys, keys that are prefixes of one another, an unterminated last line, no key at all"""
    from panfeed_amd.downstream import RowFilter
    text = b"h1\tx\tAAA\nab\t1\tkey\nabc\t2\tkey2\nab\t3\tkex\n\t\tkey\nabc\tlast\tkey"
    p = tmp_path / "t.tsv"
    p.write_bytes(text)
    f = RowFilter(["key"], first_field=False)
    assert f.filter_file(str(p)) == (b"h1\tx\tAAA\n", b"ab\t1\tkey\n\t\tkey\nabc\tlast\tkey\n")
    f.close()
    f = RowFilter(["ab", ""], first_field=True)
    assert f.filter_file(str(p))[1] == b"ab\t1\tkey\nab\t3\tkex\n\t\tkey\n"
    f.close()
    f = RowFilter([], first_field=True)
    assert f.filter_file(str(p))[1] == b""
    f.close()


def test_numeric_cluster_ids_with_an_na(tmp_path):
    """a cluster column pandas reads as float with an NA-like name in it: every NaN cell is a new float object
    (`tolist()`), so a dict keyed by them missed its own keys (KeyError: nan).  Expected texts: the reference's own
    `main()`s on these files, run in the build container (its `isin(bunch)` does not select the NaN rows of kmers.tsv,
    get_kmers.py:131-134; get_clusters prints the NaN cluster)"""
    kh = "cluster\tk-mer\thashed_pattern\n" + "".join(f"{c}\t{k}\t{h}\n" for c, k, h in [
        ("7", "", "H0"), ("7", "ACGTA", "H1"), ("NA", "", "H2"), ("NA", "CCGTA", "H1"), ("12", "GGGTA", "H3"), ("NA", "TTGTA", "H1")])
    ks = ("cluster\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\tgene_start\tgene_end\tstrand\tk-mer\n"
          "7\ts1\tg\tc\t1\t1\t6\t0\t5\t1\tACGTA\nNA\ts1\tg\tc\t1\t9\t14\t0\t5\t1\tCCGTA\n12\ts1\tg\tc\t1\t1\t6\t0\t5\t1\tGGGTA\n")
    assoc = "variant\tlrt-pvalue\nH1\t0.001\nH3\t0.5\n"
    (tmp_path / "kh.tsv").write_text(kh)
    (tmp_path / "ks.tsv").write_text(ks)
    (tmp_path / "a.tsv").write_text(assoc)
    got, rc = _run("get_kmers", ["-a", str(tmp_path / "a.tsv"), "-p", str(tmp_path / "kh.tsv"), "-k", str(tmp_path / "ks.tsv"), "-t", "0.01"])
    assert rc == 0
    # (the reference prints the cluster as 7.0: it parses the whole of kmers.tsv, where the 'NA' makes the column float, and
    # filters afterwards; here only the kept rows are parsed -- DESIGN.md's known difference for names that read as numbers)
    assert got.replace("\n7\t", "\n7.0\t") == (
        "cluster\tk-mer\thashed_pattern\tlrt-pvalue\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\t"
        "contig_end\tgene_start\tgene_end\tstrand\n7.0\tACGTA\tH1\t0.001\ts1\tg\tc\t1\t1\t6\t0\t5\t1\n")
    got, rc = _run("get_clusters", ["-a", str(tmp_path / "a.tsv"), "-p", str(tmp_path / "kh.tsv"), "-t", "0.01"])
    assert rc == 0 and sorted(got.split()) == ["7.0", "nan"]


def test_scan_out_of_memory_fails_cleanly(tmp_path):
    """pf_debug_limit_alloc below the scan's candidate buffer (a million positions at least): the scan fails as out of
    memory, the filter still closes, and with the limit lifted fresh filters give the reference's output again"""
    from panfeed_amd import _lib
    from panfeed_amd.downstream import RowFilter
    fx = FIX[0]
    paths, pa = _files(tmp_path, fx)
    run = next(r for r in fx["runs"] if r["tool"] == "get_kmers" and r["args"] == ["-t", "0.01"])
    L = _lib.load()
    f = RowFilter(["x"], first_field=True)
    try:
        _lib.check(L.pf_debug_limit_alloc(1 << 20, None))
        with pytest.raises(_lib.PanfeedHipError) as ei:
            f.filter_file(paths["kmers.tsv"])
        assert ei.value.status == _lib.ERR_OOM
        f.close()
    finally:
        _lib.check(L.pf_debug_limit_alloc(0, None))
    got, rc = _run("get_kmers", ["-a", pa, "-p", paths["kmers_to_hashes.tsv"], "-k", paths["kmers.tsv"], "-t", "0.01"])
    assert rc == 0 and got == run["stdout"]
