"""K-mer content edges on the GPU (the generators and the model are tests/kmer_content.py).  Uniformly random bases
never make a window that is, or nearly is, its own reverse complement, never repeat a k-mer inside a sequence and
never differ by trailing 'A's alone, so the branches only such content reaches are entered here, at every key width:

* window_keys' canonical choice decided below the first key word, and exact ties (near- and exact palindromes);
* table_update with one key in every lane of every wave (homopolymers, tandem repeats), and the forward and reverse
  key of one window being equal in non-canonical mode ((AT)n at even k);
* length as part of a sequence's identity (X, X + 'A', X + 'AAAA': equal packed words);
* a sequence beside its reverse complement (every key shared, no unit shared);
* the overflow retry's extrapolation on a cluster whose keys come late, and the learned partition line after batches
  that taught it the opposite.

Expected side: the CPU oracle text for text (pinned to the reference on this content by test_content_golden.py), and
kmer_content.check_kmers / pattern_model.check_rows, which need neither the oracle nor the library."""
import numpy as np
import pytest

import kmer_content as kc
import pattern_model as pm
from test_gpu_parity import _device_kmers_tsv, _diverse_records, _oracle_texts

pytestmark = pytest.mark.gpu

SWEEP_K = sorted(set(range(2, 127, 2)) | {1, 31, 33, 63, 65, 93, 95, 125})
NONCANON_K = [2, 8, 31, 32, 62, 64, 94, 96, 126]
CONFIGS = (dict(), dict(unit_dedup=False), dict(dedup=False))
SMALL_SCRATCH = dict(max_items=64)       # a cluster pair is a few work items; the default scratch is most of an engine's cost


def _assert_texts(out, expect, what):
    ek, ekh, ehp = expect
    assert out.hashes_to_patterns == ehp, f"{what}: hashes_to_patterns.tsv"
    assert out.kmers_to_hashes == ekh, f"{what}: kmers_to_hashes.tsv"
    assert out.kmers_tsv == ek, f"{what}: kmers.tsv"


def _sweep(k, canon):
    """the cluster pair of k with two targets (the exact palindrome's strain and the reverse complement's) through the
    three engine configurations, with the default filter against the oracle and with patfilt=False, maf=0.0 against
    the oracle and the model.  (An engine is made for one k and one filter: none outlives its case.)"""
    from panfeed_amd.engine import Engine
    recs, names, kinds = kc.content_clusters(k)
    S = len(names)
    stroi = {kinds[0]["pal0"], kinds[0]["rc"]}
    models = kc.model_clusters(recs, k, canon, stroi)
    for flt in (dict(), dict(patfilt=False, maf=0.0)):
        expect, _ = _oracle_texts(recs, stroi=stroi, klength=k, canon=canon, **flt)
        for kw in CONFIGS:
            eng = Engine(klength=k, canon=canon, max_strains=(S + 31) // 32 * 32, stroi=stroi, **SMALL_SCRATCH, **flt, **kw)
            out = eng.run(recs)
            eng.close()
            _assert_texts(out, expect, f"k={k} {kw} {flt}")
            if flt:
                pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, False)
                kc.check_kmers(out.kmers_to_hashes, out.hashes_to_patterns, out.kmers_tsv, recs, k, canon, stroi,
                               patfilt=False, models=models)


@pytest.mark.parametrize("k", SWEEP_K)
def test_content_sweep_canonical(k):
    _sweep(k, True)


@pytest.mark.parametrize("k", NONCANON_K)
def test_content_sweep_both_strands(k):
    _sweep(k, False)


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "both_strands"])
@pytest.mark.parametrize("k", [31, 64])
def test_one_key_in_every_lane_of_every_wave(k, canon):
    """A x 6000 and (AT) x 3000 as whole sequences among 40 unique alleles: for dozens of units all 64 lanes of all waves
    insert the same key (table_update's lost-race path); in non-canonical mode at k = 64 both keys of every (AT)n window
    are equal, with ordinals 2p and 2p + 1.  Few work items per sub-batch, key binning on and off."""
    from panfeed_amd.engine import Engine
    rng = np.random.default_rng(k)
    S = 200
    alleles = [(f"u{i}", kc.rand_seq(rng, 700 + 13 * i)) for i in range(40)]
    alleles[7:7] = [("A6000", b"A" * 6000)]
    alleles[23:23] = [("AT3000", b"AT" * 3000)]
    names = kc.strain_names(S, "w")
    recs = [kc.cluster("g_wave", names, alleles), kc.cluster("g_wave_rev", names, alleles[::-1])]
    stroi = {names[7]}                                       # the homopolymer's strain
    flt = dict(patfilt=False, maf=0.0)
    expect, _ = _oracle_texts(recs, stroi=stroi, klength=k, canon=canon, **flt)
    models = kc.model_clusters(recs, k, canon, stroi)
    for binning in (True, False):
        eng = Engine(klength=k, canon=canon, max_strains=S + 24, stroi=stroi, key_binning=binning, max_items=24, **flt)
        out = eng.run(recs)
        eng.close()
        _assert_texts(out, expect, f"binning={binning}")
        kc.check_kmers(out.kmers_to_hashes, out.hashes_to_patterns, out.kmers_tsv, recs, k, canon, stroi, patfilt=False,
                       models=models)


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "both_strands"])
@pytest.mark.parametrize("k", [32, 64, 126])
def test_kmers_tsv_device_on_palindromes_and_a_reverse_complement_pair(k, canon):
    """every strain a target on the palindrome cluster (ties, choices made in the second key word, a sequence beside
    its reverse complement): the strand column written by strand_bits_kernel / kt_text_kernel equals the host
    renderer's, the oracle's and the model's"""
    from panfeed_amd.engine import Engine
    recs, names, _ = kc.content_clusters(k)
    recs = recs[:1]
    stroi = set(names)
    eng = Engine(klength=k, canon=canon, max_strains=64, stroi=stroi, maf=0.0, **SMALL_SCRATCH)
    text, hb = _device_kmers_tsv(eng, recs, chunk=100_000)
    host = eng._render_targets(hb, hb.targets)
    eng.close()
    assert text == host
    (ek, _, _), _ = _oracle_texts(recs, stroi=stroi, klength=k, canon=canon, maf=0.0)
    assert text == ek
    assert text.split("\n")[:-1] == [r for m in kc.model_clusters(recs, k, canon, stroi) for r in m.rows]


def test_back_loaded_cluster_overflows_twice():
    """The retry after a table overflow extrapolates from how far the scan had come when the table was full, assuming
    that keys arrive at an even rate or earlier.  Here they arrive late: 16 tandem-repeat sequences first, then 36 that
    start with 500 bases of repeat and go on with 1 000 unique ones -- about 36 000 keys for a table of 7 424.  A fresh
    context starts a cluster of more than 24 distinct sequences as one partition.  Of its 52 x 23 = 1 196 units the
    first ~370 (sequence by sequence) or ~420 (position by position) bring next to nothing and the rest a new key in
    about two windows of three, so the table is full after ~550-590 units; the retry gets ceil(1 196 / 570 x 1.06) = 3
    partitions for keys that need five, and overflows again: n_retried >= 2 with a single cluster.  (The every-copy
    path doubles instead: 1, 2, 4, 8 partitions.)"""
    from panfeed_amd.engine import Engine
    k = 31
    rec, names = kc.back_loaded_cluster(16, 36, 1500, head=500, seed=5)
    S = len(names)
    expect, st = _oracle_texts([rec], klength=k, maf=0.0)
    assert st["unique_kmers"] > 4 * 7424
    for kw in CONFIGS:
        eng = Engine(klength=k, max_strains=(S + 31) // 32 * 32, maf=0.0, **kw)
        out = eng.run([rec])
        eng.close()
        print("back-loaded:", kw, {f: out.timing[f] for f in ("n_retried", "n_items", "n_dedup_clusters")})
        _assert_texts(out, expect, f"back-loaded {kw}")
        assert out.stats["unique_kmers"] == st["unique_kmers"]
        assert out.timing["n_retried"] >= 2, kw


def test_partition_line_learned_from_repeats_meets_diverse_clusters():
    """a context whose first batch was repeat-heavy clusters (a further distinct sequence brings next to no keys) sizes
    the partitions of the diverse clusters that follow by that; whatever it learned, the files are the oracle's"""
    from panfeed_amd.engine import Engine
    k = 31
    div, names = _diverse_records(48, 1500, seed=123)
    rng = np.random.default_rng(7)
    rep = []
    for i in range(16):
        al = kc.repeats(rng, k) + [(f"r{j}", (kc.rand_seq(rng, 3 + j) * 400)[:1000 + 10 * i]) for j in range(6)]
        rep.append(kc.cluster(f"rep{i:02d}", names, kc._distinct(al)))
    expect, st = _oracle_texts(rep + div, klength=k, maf=0.0)
    eng = Engine(klength=k, max_strains=64, maf=0.0)
    out1 = eng.run(rep)
    out2 = eng.run(div)
    eng.close()
    print("learned:", out1.timing["n_retried"], out2.timing["n_retried"], out2.timing["n_items"])
    assert out1.kmers_to_hashes + out2.kmers_to_hashes == expect[1]
    assert out1.hashes_to_patterns + out2.hashes_to_patterns == expect[2]
