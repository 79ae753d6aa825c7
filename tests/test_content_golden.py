"""Outputs of the reference itself (tests/golden/content.json.gz, written by tools/gen_golden.py content) on the k-mer
content of tests/kmer_content.py: near-palindromes whose strands first differ at chosen bases (the canonical choice
decided in the second key word, and ties), homopolymers and tandem repeats that fill whole units with one key, sequences
that differ only by trailing 'A's, a sequence beside its reverse complement; k of one to four key words, canonical and
not.  The oracle against them without a GPU, the model of kmer_content.py against them (which pins the model to the
reference), and the conditions the fixture exists for; Engine.run against them with a GPU."""
import numpy as np
import pytest

import kmer_content as kc
import numpy_packer
import pattern_model as pm
from conftest import case_ids, case_records, load_cases
from test_oracle_golden import run_oracle

CASES = load_cases("content.json.gz")
FILES = ("kmers_to_hashes.tsv", "hashes_to_patterns.tsv", "kmers.tsv")


def _body(text):
    return text[text.index("\n") + 1:]


def _models(case):
    o = case["opts"]
    return kc.model_clusters(case_records(case), o["klength"], o["canon"], set(o["stroi"] or ()))


def test_fixture_holds_the_cases_it_is_for():
    """conditions on the inputs, by the model's classifier: which key word decides the canonical choice, ties, units
    of one key, equal key pairs, equal packed words of different lengths"""
    decided = {}          # KW -> set of (word, reverse_smaller)
    low_bit_31 = {}       # KW -> directions of a window decided in word 1 at base 31 by its low bit alone
    ties, one_key, equal_noncanon = set(), set(), 0
    for case in CASES:
        o = case["opts"]
        KW = kc.key_words(o["klength"])
        for m in _models(case):
            for cls, n in m.classes.items():
                if cls is None:
                    if m.equal_pairs:
                        ties.add(KW)
                    continue
                word, rev_smaller, p, low_only = cls
                decided.setdefault(KW, set()).add((word, rev_smaller))
                if word == 1 and p == 31 and low_only:
                    low_bit_31.setdefault(KW, set()).add(rev_smaller)
            if m.one_key_units:
                one_key.add(KW)
            if not o["canon"]:
                equal_noncanon += m.equal_pairs
    for KW in (1, 2, 3, 4):
        assert {(0, False), (0, True)} <= decided[KW], f"KW {KW}: word 0 in both directions"
        assert KW in ties, f"KW {KW}: an exact tie"
        assert KW in one_key, f"KW {KW}: a unit of one key"
    for KW in (3, 4):
        assert {(1, False), (1, True)} <= decided[KW], f"KW {KW}: word 1 in both directions"
    assert any(low_bit_31.get(KW) == {False, True} for KW in (3, 4)), "word 1 at base 31 by the low bit alone"
    # beyond the list: a key that does not fill its words (k = 95: word 0 holds one bit) is decided in word 2 as well
    assert {(2, False), (2, True)} <= decided[4]
    assert equal_noncanon > 0, "a non-canonical window whose two keys are equal"
    # sequences whose packed words are equal and whose lengths differ (A packs to 00, as padding does)
    from panfeed_amd.packing import _LUT
    pairs = 0
    for case in CASES[:1] + [c for c in CASES if c["name"] == "content_k126"]:
        seqs = list(dict.fromkeys(s.sequence for gs, _, _ in case_records(case) for v in gs.values() for s in v))
        packed = {}
        for s in seqs:
            w = numpy_packer.pack_codes(_LUT[np.frombuffer(s.encode(), np.uint8)])
            packed.setdefault(w.tobytes(), set()).add(len(s))
        pairs += sum(1 for v in packed.values() if len(v) >= 2)
    assert pairs >= 2


@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_oracle_matches_reference(case):
    got = run_oracle(case)
    exp = case["expect"]
    for f in FILES:
        assert got[f] == exp[f], f
    assert got["n_patterns"] == exp["n_patterns"]


@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_model_matches_reference(case):
    """check_kmers and the row check on the reference's own texts: the model is the reference's, not the oracle's"""
    o, exp = case["opts"], case["expect"]
    assert o["maf"] == 0.0
    kc.check_kmers(exp["kmers_to_hashes.tsv"], exp["hashes_to_patterns.tsv"], exp["kmers.tsv"], case_records(case),
                   o["klength"], o["canon"], set(o["stroi"] or ()), o["consider_missing"], o["patfilt"])
    pm.check_rows(_body(exp["hashes_to_patterns.tsv"]), _body(exp["kmers_to_hashes.tsv"]), len(case["all_strains"]),
                  o["consider_missing"])


def test_check_kmers_notices_a_wrong_strand_an_order_and_a_row():
    """the check itself: a tie given to the reverse strand, two k-mers swapped, a flipped cell"""
    case = next(c for c in CASES if c["name"] == "content_k64")
    o, exp = case["opts"], case["expect"]
    recs = case_records(case)
    args = (recs, o["klength"], o["canon"], set(o["stroi"]))
    models = kc.check_kmers(exp["kmers_to_hashes.tsv"], exp["hashes_to_patterns.tsv"], exp["kmers.tsv"], *args)
    kt = exp["kmers.tsv"].split("\n")
    tie = next(i for i, ln in enumerate(kt) if ln.endswith("\t1\t" + "AT" * 32))
    bad = kt[:tie] + [kt[tie].replace("\t1\tAT", "\t-1\tAT")] + kt[tie + 1:]
    with pytest.raises(AssertionError):
        kc.check_kmers(exp["kmers_to_hashes.tsv"], exp["hashes_to_patterns.tsv"], "\n".join(bad), *args, models=models)
    kh = exp["kmers_to_hashes.tsv"].split("\n")
    with pytest.raises(AssertionError):
        kc.check_kmers("\n".join(kh[:2] + [kh[3], kh[2]] + kh[4:]), exp["hashes_to_patterns.tsv"], exp["kmers.tsv"], *args,
                       models=models)
    hp = exp["hashes_to_patterns.tsv"].split("\n")
    name, cells = hp[2].split("\t", 1)
    flipped = cells.replace("1", "x", 1).replace("0", "1", 1).replace("x", "0", 1)
    with pytest.raises(AssertionError):
        kc.check_kmers(exp["kmers_to_hashes.tsv"], "\n".join(hp[:2] + [name + "\t" + flipped] + hp[3:]), exp["kmers.tsv"],
                       *args, models=models)


@pytest.mark.gpu
@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "nodedup"])
@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_engine_matches_reference(case, dedup):
    from panfeed_amd.engine import Engine, KMERS_TSV_HEADER, KMERS_TO_HASHES_HEADER, hashes_to_patterns_header
    o = case["opts"]
    S = len(case["all_strains"])
    eng = Engine(klength=o["klength"], canon=o["canon"], consider_missing=o["consider_missing"], patfilt=o["patfilt"],
                 maf=o["maf"], max_strains=S, stroi=set(o["stroi"]) if o["stroi"] else (), dedup=dedup, max_items=64)
    out = eng.run(case_records(case))
    eng.close()
    exp = case["expect"]
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, o["consider_missing"])
    assert hashes_to_patterns_header(case["all_strains"]) + out.hashes_to_patterns == exp["hashes_to_patterns.tsv"]
    assert KMERS_TO_HASHES_HEADER + out.kmers_to_hashes == exp["kmers_to_hashes.tsv"]
    assert KMERS_TSV_HEADER + out.kmers_tsv == exp["kmers.tsv"]
    assert out.stats["patterns"] == exp["n_patterns"]
