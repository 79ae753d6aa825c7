"""Sample-count edges.  Every kernel after the scan works on rows of S samples -- the pattern bits, the MD5 image
(8 S bytes: S >> 3 whole blocks, a tail of S & 7 elements whose byte sits at (S >> 3) & 3 of a 32-sample row word, an
extra padding block when the tail is 7), the hashes_to_patterns text, the MAF cut -- so their edges are functions of S:
every S from 1 to 160, the sizes around the word, block and chunk boundaries up to the 8 192-strain ceiling, and the
ceiling itself.

Every GPU case compares all three texts with the CPU oracle, bit for bit, and runs pattern_model.check_rows (hashlib
and numpy only) on the GPU's own output.  The CPU tests of this file apply the same row check to the oracle's output
over the same lists, so the GPU comparisons rest on something that runs without a GPU, and assert that the dense list
reaches every shape of MD5 tail."""
import numpy as np
import pytest

import pattern_model as pm

gpu = pytest.mark.gpu

K = 11                                   # odd (no palindromes), short: ~90 bp sequences with six substitutions
DENSE_N = list(range(1, 161))
DENSE_W = [1, 2, 3, 4, 5]                # one engine per W, max_strains = 32 W, its 32 values of n in successive runs
SPARSE_S = [255, 256, 257, 1000, 1007, 1023, 1024, 1025, 4095, 5000, 8159, 8160, 8161, 8191, 8192]
SPARSE_MAF = [0.01, 0.05]
DENSE_FLAGS = [(False, True), (False, False), (True, True), (True, False)]       # (consider_missing, patfilt)
TARGET = "s00000"                        # column 0 of every dense cluster: always present, its rows go to kmers.tsv


def _flag_id(f):
    return ("missing" if f[0] else "plain") + ("" if f[1] else "_nopatfilt")


def _dense_ns(W):
    return [n for n in DENSE_N if (n + 31) // 32 == W]


def _n_absent(S, missing):
    """absent strains of a consider_missing case: a fifth of the columns, at least one where a present one is left"""
    return min(S - 1, max(1, S // 5)) if missing and S >= 2 else 0


def _dense_cluster(n, missing):
    nabs = _n_absent(n, missing)
    P = n - nabs
    counts = [c for c in dict.fromkeys((1, P // 2, P // 3)) if 1 <= c <= P - 1]
    counts = [c for i, c in enumerate(counts) if P - c not in counts[:i]]
    return pm.count_exact_cluster(n, K, counts, seed=1000 + n, idx=f"n{n:03d}", n_absent=nabs, keep_present=(0,))


def _sparse_cluster(S, maf, missing=False, keep_present=(-1,)):
    nabs = _n_absent(S, missing)
    return pm.count_exact_cluster(S, K, pm.edge_counts(S - nabs, maf), seed=7 * S + int(maf * 100), idx=f"S{S}",
                                  n_absent=nabs, keep_present=keep_present)


def _oracle(**kw):
    from oracle import oracle as po
    return po.OracleRun(**kw)


def _oracle_step(run, records):
    """texts of these records alone, the run-global pattern set kept"""
    run.clear_text()
    run.feed(records)
    return run.texts()


def _n_kmer_rows(kmers_to_hashes):
    return sum(1 for ln in kmers_to_hashes.split("\n")[:-1] if ln.split("\t")[1] != "")


# ------------------------------------------------------------------------------------------------ CPU
def test_dense_list_reaches_every_tail_shape():
    """thinning the lists must not quietly lose a shape: every (tail length, byte of the row word the tail sits in) of
    md5_kernel, every W mod 4 of its four-word prefetch, and the padding block of a 7-element tail at every byte"""
    shapes = {(n & 7, (n >> 3) & 3) for n in DENSE_N}
    assert shapes == {(r, b) for r in range(8) for b in range(4)}
    assert {(n + 31) // 32 % 4 for n in DENSE_N} == {0, 1, 2, 3}
    assert {W % 4 for W in DENSE_W} == {0, 1, 2, 3}
    assert sorted(n for W in DENSE_W for n in _dense_ns(W)) == DENSE_N and all(len(_dense_ns(W)) == 32 for W in DENSE_W)
    assert {(n >> 3) & 3 for n in DENSE_N if n & 7 == 7} == {0, 1, 2, 3}
    # at size: a 7-element tail in a row of 256 words, a full last word, one element into a new word / block / chunk
    assert {S & 7 for S in SPARSE_S} >= {0, 1, 7} and {S & 31 for S in SPARSE_S} >= {0, 1, 31}
    assert 8192 in SPARSE_S and 8191 in SPARSE_S


@pytest.mark.parametrize("flags", DENSE_FLAGS, ids=_flag_id)
@pytest.mark.parametrize("W", DENSE_W)
def test_row_model_holds_on_the_oracle_dense(W, flags):
    """the oracle's rows re-hash to their own names under hashlib, n = 1..160, the pattern set carried along"""
    missing, patfilt = flags
    run = _oracle(klength=K, stroi={TARGET}, consider_missing=missing, patfilt=patfilt, maf=0.0)
    known = set()
    for n in _dense_ns(W):
        cx = _dense_cluster(n, missing)
        _, kh, hp = _oracle_step(run, [cx.record])
        known = pm.check_rows(hp, kh, n, missing, known)
        if patfilt:
            assert _n_kmer_rows(kh) == pm.kept_rows(cx, 0.0, missing) == len(cx.kmer_counts)


@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("maf", SPARSE_MAF)
@pytest.mark.parametrize("S", SPARSE_S)
def test_row_model_and_kept_rows_hold_on_the_oracle_sparse(S, maf, missing):
    cx = _sparse_cluster(S, maf, missing)
    run = _oracle(klength=K, stroi={cx.names[-1]}, consider_missing=missing, maf=maf)
    kt, kh, hp = _oracle_step(run, [cx.record])
    pm.check_rows(hp, kh, S, missing)
    assert _n_kmer_rows(kh) == pm.kept_rows(cx, maf, missing)
    assert len(kt) > 0


def test_row_model_notices_a_wrong_digest_and_a_wrong_bit():
    """the check itself: a digest of other bits, a flipped cell, a short row, a hash without a row"""
    cx = _sparse_cluster(39, 0.05, True)
    run = _oracle(klength=K, consider_missing=True, maf=0.05)
    _, kh, hp = _oracle_step(run, [cx.record])
    pm.check_rows(hp, kh, 39, True)
    rows = hp.split("\n")[:-1]
    name, cells = rows[1].split("\t", 1)
    flipped = cells.replace("1", "x", 1).replace("0", "1", 1).replace("x", "0", 1)
    for bad in ("\n".join([rows[0], name + "\t" + flipped] + rows[2:]) + "\n",
                "\n".join([rows[0], name + "\t" + cells[:cells.rindex("\t")]] + rows[2:]) + "\n",
                "\n".join(rows[:1] + rows[2:]) + "\n"):
        with pytest.raises(AssertionError):
            pm.check_rows(bad, kh, 39, True)
    with pytest.raises(AssertionError):
        pm.check_rows(hp, kh, 39, False)          # NaN cells without consider_missing


# ------------------------------------------------------------------------------------------------ GPU
SMALL_SCRATCH = dict(max_items=64)       # these batches are a few work items; the default 2 048 slices of scratch are
                                         # tens of gigabytes at W = 256, and allocating them is most of an engine's cost


def _engine(**kw):
    from panfeed_amd.engine import Engine
    return Engine(**kw)


def _assert_texts(out, expect, what):
    ek, ekh, ehp = expect
    assert out.hashes_to_patterns == ehp, f"{what}: hashes_to_patterns.tsv"
    assert out.kmers_to_hashes == ekh, f"{what}: kmers_to_hashes.tsv"
    assert out.kmers_tsv == ek, f"{what}: kmers.tsv"


@gpu
@pytest.mark.parametrize("flags", DENSE_FLAGS, ids=_flag_id)
@pytest.mark.parametrize("W", DENSE_W)
def test_dense_sweep(W, flags):
    """n = 32 (W - 1) + 1 .. 32 W on one engine of max_strains = 32 W, one cluster per run call, against one oracle run
    fed in the same order: every tail length at every byte of the last row word, int64 and float64 rows, with and
    without NaN cells"""
    missing, patfilt = flags
    opts = dict(klength=K, stroi={TARGET}, consider_missing=missing, patfilt=patfilt, maf=0.0)
    run = _oracle(**opts)
    eng = _engine(max_strains=32 * W, **opts)
    assert eng.W == W
    known = set()
    wrong = []
    for n in _dense_ns(W):
        cx = _dense_cluster(n, missing)
        expect = _oracle_step(run, [cx.record])
        out = eng.run([cx.record])
        try:
            known = pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, n, missing, known)
            _assert_texts(out, expect, f"n={n}")
            assert len(out.kmers_tsv) > 0
        except AssertionError as e:
            wrong.append(f"n={n} (tail {n & 7}, byte {(n >> 3) & 3}): {str(e).splitlines()[0][:300]}")
            known |= {ln.split("\t")[2] for ln in expect[1].split("\n")[:-1]}
    eng.close()
    assert not wrong, f"{len(wrong)} of 32 sample counts differ:\n" + "\n".join(wrong)


@gpu
@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("maf", SPARSE_MAF)
@pytest.mark.parametrize("S", SPARSE_S)
def test_sparse_sweep(S, maf, missing):
    """count-exact clusters at size: the counts on either side of the MAF cut and of one half, the number of kept rows
    from the reference's float arithmetic alone, a target strain in the last column"""
    cx = _sparse_cluster(S, maf, missing)
    opts = dict(klength=K, stroi={cx.names[-1]}, consider_missing=missing, maf=maf)
    expect = _oracle_step(_oracle(**opts), [cx.record])
    eng = _engine(max_strains=(S + 31) // 32 * 32, **SMALL_SCRATCH, **opts)
    out = eng.run([cx.record])
    eng.close()
    assert _n_kmer_rows(out.kmers_to_hashes) == pm.kept_rows(cx, maf, missing)
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, missing)
    _assert_texts(out, expect, f"S={S}")
    assert len(out.kmers_tsv) > 0


def _max_strains_cases():
    # S + 160 leaves the row five words short of W.  8191 + 160 is above the ceiling, so that size takes the ceiling
    # itself there, and 8032 = 8192 - 160 is the row five words short of the ceiling's W = 256.
    out = []
    for S in (39, 1007, 8191, 8032):
        for ms in dict.fromkeys((S, (S + 31) // 32 * 32, min(S + 160, 8192))):
            out.append((S, ms))
    return out


@gpu
@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("S,max_strains", _max_strains_cases())
def test_max_strains_exact_rounded_and_slack(S, max_strains, missing):
    """max_strains need not be a multiple of 32 nor close to the cluster's own count: exactly S (odd), rounded up to
    a whole word, and 160 beyond (rows five words short of W)"""
    cx = _sparse_cluster(S, 0.01, missing)
    opts = dict(klength=K, stroi={cx.names[-1]}, consider_missing=missing, maf=0.01)
    expect = _oracle_step(_oracle(**opts), [cx.record])
    eng = _engine(max_strains=max_strains, **SMALL_SCRATCH, **opts)
    assert eng.W == (max_strains + 31) // 32
    out = eng.run([cx.record])
    eng.close()
    assert _n_kmer_rows(out.kmers_to_hashes) == pm.kept_rows(cx, 0.01, missing)
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, missing)
    _assert_texts(out, expect, f"S={S} max_strains={max_strains}")


@gpu
@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "nodedup"])
@pytest.mark.parametrize("S", [8191, 8192])
def test_ceiling(S, dedup):
    """max_strains = 8192, W = 256 = MAX_CHUNKS: the last elements of the chunk arrays, bit 31 of word 255 (S = 8192:
    the target strain's column), and the two sides of the sample-set matrix's limit D * ceil4(W) <= DEDUP_MROWS --
    16 distinct sequences fit it, 17 go through the wide class"""
    from test_gpu_parity import _allele_cluster
    cx = _sparse_cluster(S, 0.01)
    rng = np.random.default_rng(S)
    recs = [_allele_cluster(rng, f"d{D}", cx.names, D, 90) for D in (16, 17)]
    recs.append(cx.record)
    last = cx.names[-1]
    opts = dict(klength=K, stroi={last}, maf=0.01)
    run = _oracle(**opts)
    expect = _oracle_step(run, recs)
    eng = _engine(max_strains=8192, dedup=dedup, **opts)          # the default scratch, as a run at the ceiling has it
    assert eng.W == 256
    out = eng.run(recs)
    eng.close()
    if dedup:
        assert out.timing["n_dedup_clusters"] == 3 and out.timing["n_wide_clusters"] == 1
    else:
        assert out.timing["n_dedup_clusters"] == 0
    pm.check_rows(out.hashes_to_patterns, out.kmers_to_hashes, S, False)
    _assert_texts(out, expect, f"S={S}")
    assert out.stats["unique_kmers"] == run.stats()["unique_kmers"]
    assert f"\t{last}\t" in out.kmers_tsv
    if S == 8192:
        # the last column's cell is bit 31 of word 255: set in some rows, clear in others
        ends = {ln[-2:] for ln in out.hashes_to_patterns.split("\n")[:-1]}
        assert ends == {"\t0", "\t1"}


@gpu
def test_one_past_the_ceiling_is_refused():
    from panfeed_amd import _lib
    with pytest.raises(_lib.PanfeedHipError) as e:
        _engine(klength=K, max_strains=8193)
    assert e.value.status == _lib.ERR_ARG
    eng = _engine(klength=K, max_strains=8192)
    eng.close()


@gpu
@pytest.mark.parametrize("S", [1007, 8191])
def test_device_rendered_text_at_a_seven_cell_tail(S):
    """hp_text_kernel / hp_rowlen_kernel with a NaN mask whose last cells are a 7-element tail (S = 8191: in the last
    of 256 words): the device's text equals the host renderers' and the oracle's; two submits, the pool growing"""
    from panfeed_amd.packing import build_batch_native
    a = _sparse_cluster(S, 0.01, True)
    b = pm.count_exact_cluster(S, K, pm.edge_counts(S - _n_absent(S, True), 0.05), seed=S + 1, idx="second",
                               n_absent=_n_absent(S, True))
    opts = dict(klength=K, consider_missing=True, maf=0.01)
    run = _oracle(**opts)
    eng = _engine(max_strains=S, **SMALL_SCRATCH, **opts)
    known = set()
    for i, cx in enumerate((a, b)):
        _, ekh, ehp = _oracle_step(run, [cx.record])
        hb = build_batch_native([cx.record], eng.k, eng.canon, eng.W, first_ordinal=i)
        eng.submit_host_batch(hb)
        kh, hp = eng.render_device(hb)
        kh, hp = bytes(kh).decode(), bytes(hp).decode()
        host = eng._render(hb, eng.fetch())
        assert "\t\t" in hp or "\t\n" in hp                  # NaN cells
        known = pm.check_rows(hp, kh, S, True, known)
        assert hp == host.hashes_to_patterns and kh == host.kmers_to_hashes
        assert hp == ehp and kh == ekh
    eng.close()
