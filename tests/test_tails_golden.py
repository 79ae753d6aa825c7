"""Outputs of the reference itself (tests/golden/tails.json.gz, written by tools/gen_golden.py tails) at the sample
counts where the row kernels change shape: 7-element MD5 tails (S = 7, 15, 39, 1007, 8191), the float64 MAF boundary at
S = 1000, NaN cells in a 126-block image, 157-word rows with a target strain, the 8 192-strain ceiling.  The oracle
against them without a GPU; Engine.run against them with one, with and without the identical-sequence shortcut."""
import pytest

import pattern_model as pm
from conftest import case_ids, case_records, load_cases
from test_oracle_golden import run_oracle

CASES = load_cases("tails.json.gz")
FILES = ("kmers_to_hashes.tsv", "hashes_to_patterns.tsv", "kmers.tsv")


def _body(text):
    return text[text.index("\n") + 1:]


def test_fixture_holds_the_cases_it_is_for():
    sizes = {len(c["all_strains"]) for c in CASES}
    assert sizes >= {7, 15, 39, 1000, 1007, 5000, 8191, 8192}
    by = {c["name"]: c for c in CASES}
    # counts 9 and 991 of 1 000 go at maf 0.01, 10 and 990 stay (panfeed.py:190-200): rows of the reference's own text
    hp = _body(by["s1000_maf_boundary"]["expect"]["hashes_to_patterns.tsv"]).split("\n")[:-1]
    ones = sorted(ln.split("\t")[1:].count("1") for ln in hp)
    assert 10 in ones and 990 in ones and 9 not in ones and 991 not in ones
    assert "\t\t" in by["s1007_missing"]["expect"]["hashes_to_patterns.tsv"]
    assert len(_body(by["s5000_k21_target"]["expect"]["kmers.tsv"])) > 0


@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_oracle_matches_reference(case):
    got = run_oracle(case)
    exp = case["expect"]
    for f in FILES:
        assert got[f] == exp[f], f
    assert got["n_patterns"] == exp["n_patterns"]
    # and the reference's own rows re-hash to their names under the independent row check
    pm.check_rows(_body(exp["hashes_to_patterns.tsv"]), _body(exp["kmers_to_hashes.tsv"]), len(case["all_strains"]),
                  case["opts"]["consider_missing"])


@pytest.mark.gpu
@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "nodedup"])
@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_engine_matches_reference(case, dedup):
    from panfeed_amd.engine import Engine, KMERS_TSV_HEADER, KMERS_TO_HASHES_HEADER, hashes_to_patterns_header
    o = case["opts"]
    S = len(case["all_strains"])
    eng = Engine(klength=o["klength"], canon=o["canon"], consider_missing=o["consider_missing"], patfilt=o["patfilt"],
                 maf=o["maf"], max_strains=S, stroi=set(o["stroi"]) if o["stroi"] else (), dedup=dedup,
                 max_items=64)          # one cluster each: the default scratch of 2 048 work items is gigabytes at this W
    out = eng.run(case_records(case))
    eng.close()
    exp = case["expect"]
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, o["consider_missing"])
    assert hashes_to_patterns_header(case["all_strains"]) + out.hashes_to_patterns == exp["hashes_to_patterns.tsv"]
    assert KMERS_TO_HASHES_HEADER + out.kmers_to_hashes == exp["kmers_to_hashes.tsv"]
    assert KMERS_TSV_HEADER + out.kmers_tsv == exp["kmers.tsv"]
    assert out.stats["patterns"] == exp["n_patterns"]
