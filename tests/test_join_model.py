"""The device join of panfeed-get-kmers without a device (tests/join_tables.py): the model -- the package's host half,
`rendered_texts` among it, with a Python stand-in for the kernels -- reproduces what the reference's own get_kmers printed
for every golden run, and the plainness rule flags every row that pandas' read_csv -> to_csv does not print as it stands."""
import gzip
import io
import json
import os

import pandas as pd
import pytest

import join_tables as jt
from conftest import GOLDEN, all_cases

with gzip.open(os.path.join(GOLDEN, "n4.json.gz"), "rb") as _fh:
    FIX = json.loads(_fh.read().decode())["fixtures"]
CASES = {c["name"]: c for c in all_cases()}
RUNS = [(f["case"], i) for f in FIX for i, r in enumerate(f["runs"]) if r["tool"] == "get_kmers" and "--only-passing" not in r["args"]]


def _option(args, name, default, kind):
    return kind(args[args.index(name) + 1]) if name in args else default


def test_every_right_join_run_is_covered():
    assert len(RUNS) == 16


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{i}" for c, i in RUNS])
def test_join_model_equals_reference(tmp_path, case, i):
    fx = next(f for f in FIX if f["case"] == case)
    run = fx["runs"][i]
    exp = CASES[case]["expect"]
    pa = tmp_path / "assoc.tsv"
    pa.write_text(fx["associations"])
    per = _option(run["args"], "--clusters-per-iteration", 15, int)
    got, routes = jt.join_model(str(pa), exp["kmers_to_hashes.tsv"].encode(), exp["kmers.tsv"].encode(),
                                threshold=_option(run["args"], "-t", 1.0, float), column=_option(run["args"], "-c", "lrt-pvalue", str),
                                per_iteration=per)
    assert all(routes), "a bunch of the golden files is not plain"
    if len(routes) <= 1:
        assert got == run["stdout"]
    else:
        gl, el = got.splitlines(), run["stdout"].splitlines()
        assert gl[:1] == el[:1] and sorted(gl[1:]) == sorted(el[1:])


PLAIN_ROW = [b"group_17", b"12345_6#7", b"gene_1", b"NODE_1", b"1", b"10", b"40", b"0", b"30", b"-1", b"ACGTACGTAC"]
HEADER = (b"cluster\tstrain\tfeature_id\tcontig\tfeature_strand\tcontig_start\tcontig_end\tgene_start\tgene_end\tstrand\tk-mer\n")
AWKWARD = ([b""] + list(jt.NA_STRINGS) +
           [b"007", b"1e3", b".5", b"+1", b"-0", b"1_0", b"0x1F", b"True", b"INF", b"E", b"1234567890123456789",
            b" x", b"x ", b" 1", b"1 ", b'a"b', b"a\rb", b"caf\xc3\xa9", b"\xff"])


def test_plain_rows_are_not_flagged():
    assert jt.plainness(b"\t".join(PLAIN_ROW)) == 0
    assert jt.plainness(b"\t".join([b"c", b"s", b"f", b"n", b"0", b"-5", b"123456789012345678", b"7", b"8", b"9", b"k"])) == 0


def _roundtrip(table):
    try:
        return pd.read_csv(io.BytesIO(table), sep="\t").to_csv(sep="\t", index=False).encode()
    except Exception:
        return None


@pytest.mark.parametrize("col", range(11))
def test_plainness_is_conservative_against_pandas(col):
    """each awkward value in column `col` of the middle row of an otherwise plain three-row table: when pandas does not
    give the table's bytes back, the rule flags the row"""
    assert jt.NA_STRINGS == tuple(sorted(v.encode() for v in pd._libs.parsers.STR_NA_VALUES if v))
    changed = 0
    for v in AWKWARD:
        row = list(PLAIN_ROW)
        row[col] = v
        line = b"\t".join(row)
        table = HEADER + b"\t".join(PLAIN_ROW) + b"\n" + line + b"\n" + b"\t".join(PLAIN_ROW) + b"\n"
        if _roundtrip(table) != table:
            changed += 1
            assert jt.plainness(line), (col, v)
    assert changed >= 10


@pytest.mark.parametrize("per", [1, 2, 15])
@pytest.mark.parametrize("int_column", [False, True], ids=["text_columns", "int_column"])
@pytest.mark.parametrize("only_passing", [False, True], ids=["right", "left"])
def test_model_equals_the_pandas_statements_on_the_handmade_table(tmp_path, per, int_column, only_passing):
    """an associations file with an integer column makes the two renderings differ; bunches with and without an
    unmatched row: the model's text is what the pandas statements print"""
    t = jt.handmade(int_column=int_column)
    pa = tmp_path / "assoc.tsv"
    pa.write_text(t["assoc"])
    got, routes = jt.join_model(str(pa), t["kh"], t["kmers"], threshold=0.5, per_iteration=per, only_passing=only_passing)
    host, _ = jt.join_model(str(pa), t["kh"], t["kmers"], threshold=0.5, per_iteration=per, only_passing=only_passing, host=True)
    assert routes and all(routes)
    assert got == host
    if int_column and per == 1 and not only_passing:
        assert "\tCCA\tH5\t1e-06\t7\t" in got and "\tACG\tH1\t0.01\t3.0\t" in got      # both renderings were used


def test_handmade_table_puts_rows_on_every_place():
    begins, ends = jt.vector_places(jt.handmade()["kmers"])
    assert begins == set(range(16)) and ends == set(range(16))
