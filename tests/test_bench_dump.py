"""bench.py --dump-outputs without a GPU: OutputDump fed pf_fetch-shaped results (rows placed out of cluster order, as
the library's arenas place them) must write every row where the caller's order puts it, keyed by digests, and keep a
sample within its byte budget; --full is off by default and --steps is checked."""
import ctypes as C
import os

import numpy as np
import pytest

import bench
from panfeed_amd import _lib


class FakeBatchResult:
    """what pf_fetch hands over for one batch: n clusters, their kept k-mers stored in a shuffled cluster order"""

    def __init__(self, n, kw=1, W=2, P=40, pid0=0, seed=0):
        rng = np.random.default_rng(seed)
        self.n, self.kw, self.W, self.P = n, kw, W, P
        self.cnt = rng.integers(0, 12, n).astype(np.uint32)
        self.off = np.zeros(n, np.uint64)
        o = 0
        for c in rng.permutation(n):
            self.off[c] = o
            o += int(self.cnt[c])
        tot = int(self.cnt.sum())
        self.keys = rng.integers(0, 2 ** 63, tot * kw, dtype=np.uint64)
        self.kpid = rng.integers(0, P, tot).astype(np.uint32)
        self.uniq = rng.integers(0, 30, n).astype(np.uint32)
        self.cpat = rng.integers(0, P, n).astype(np.uint32)
        self.cpat[0] = 0xFFFFFFFF                       # a cluster without a row of its own
        self.md5 = rng.integers(0, 256, P * 16).astype(np.uint8)
        self.new = rng.permutation(np.arange(pid0, P, dtype=np.uint32))
        self.first_seen = rng.integers(0, 2 ** 40, P, dtype=np.uint64)
        self.pat_n = np.full(P, 37, np.uint32)
        self.bits = rng.integers(0, 2 ** 32, P * W, dtype=np.uint64).astype(np.uint32)
        self.n_clusters = n                             # (the DeviceBatch side of it)

    def result_checksum(self):
        return (2 ** 64 - 1, 7, int(self.cnt.sum()))

    def fetch(self):
        r = _lib.Result()
        p = (lambda a, t: a.ctypes.data_as(C.POINTER(t)))
        r.cluster_kmer_off, r.cluster_kmer_cnt = p(self.off, C.c_uint64), p(self.cnt, C.c_uint32)
        r.cluster_unique, r.cluster_pattern = p(self.uniq, C.c_uint32), p(self.cpat, C.c_uint32)
        r.kmer_key, r.kmer_pattern = p(self.keys, C.c_uint64), p(self.kpid, C.c_uint32)
        r.pattern_md5, r.new_pattern_id = p(self.md5, C.c_uint8), p(self.new, C.c_uint32)
        r.pattern_first_seen, r.pattern_n = p(self.first_seen, C.c_uint64), p(self.pat_n, C.c_uint32)
        r.pattern_bits = p(self.bits, C.c_uint32)
        r.n_patterns, r.n_new_patterns, r.key_words, r.W = self.P, len(self.new), self.kw, self.W
        r.n_kept = int(self.cnt.sum())
        return r


def _check(outdir, batches):
    a = {f[:-4]: np.load(os.path.join(outdir, f)) for f in os.listdir(outdir)}
    assert all(x.dtype == np.float64 for x in a.values())
    cbase = np.cumsum([0] + [b.n for b in batches])
    pbase = np.cumsum([0] + [len(b.new) for b in batches])

    def batch_of(base, i):
        j = int(np.searchsorted(base, i, side="right")) - 1
        return batches[j], i - int(base[j])
    for row in a["clusters"]:
        b, c = batch_of(cbase, int(row[0]))
        assert row[1] == b.cnt[c] and row[2] == b.uniq[c]
        want = [-1.0] * 4 if b.cpat[c] == 0xFFFFFFFF else b.md5.view("<u4").reshape(-1, 4)[b.cpat[c]]
        assert list(row[3:7]) == list(want)
    for row in a["kmers"]:
        b, c = batch_of(cbase, int(row[0]))
        pos = int(row[1])
        assert pos < b.cnt[c]
        src = int(b.off[c]) + pos
        key = b.keys.reshape(-1, b.kw)[src]
        assert [int(x) for x in row[2:2 + 2 * b.kw]] == [v for k in key for v in (int(k) >> 32, int(k) & 0xFFFFFFFF)]
        assert list(row[2 + 2 * b.kw:]) == list(b.md5.view("<u4").reshape(-1, 4)[b.kpid[src]])
    for row in a["patterns"]:
        b, i = batch_of(pbase, int(row[0]))
        pid = b.new[i]
        assert list(row[1:5]) == list(b.md5.view("<u4").reshape(-1, 4)[pid])
        assert int(row[5]) * 2 ** 32 + int(row[6]) == int(b.first_seen[pid]) and row[7] == 37
        assert list(row[8:]) == list(b.bits.reshape(-1, b.W)[pid])
    assert a["result_checksums"].shape == (len(batches), 6)
    assert list(a["result_checksums"][0, :2]) == [2 ** 32 - 1, 2 ** 32 - 1]
    return a


@pytest.mark.parametrize("budget", [bench.DUMP_BYTES, 6000])
def test_dump_rows_in_caller_order(tmp_path, budget):
    b = FakeBatchResult(200, kw=2, W=3)
    d = bench.OutputDump(b.n, int(b.cnt.sum()), len(b.new), budget=budget)
    d.add(b, b)
    total = d.write(str(tmp_path), counts=[1, 2, 3])
    a = _check(str(tmp_path), [b])
    if budget == bench.DUMP_BYTES:
        assert len(a["clusters"]) == b.n and len(a["kmers"]) == int(b.cnt.sum()) and len(a["patterns"]) == len(b.new)
    else:                                                # sampled: within the budget, the same rows every time
        assert len(a["kmers"]) < int(b.cnt.sum()) and total <= budget + 1000
        d2 = bench.OutputDump(b.n, int(b.cnt.sum()), len(b.new), budget=budget)
        d2.add(b, b)
        d2.write(str(tmp_path / "again"))
        assert np.array_equal(np.load(tmp_path / "again" / "kmers.npy"), a["kmers"])


def test_dump_over_several_batches(tmp_path):
    bs = [FakeBatchResult(60, seed=1), FakeBatchResult(90, seed=2, pid0=15)]
    d = bench.OutputDump(150, sum(int(b.cnt.sum()) for b in bs), sum(len(b.new) for b in bs), budget=4000)
    for b in bs:
        d.add(b, b)
    d.write(str(tmp_path))
    a = _check(str(tmp_path), bs)
    assert a["kmers"][:, 0].max() >= 60                 # rows of the second batch, numbered after the first's clusters


def test_plain_run_is_the_default():
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.steps == 7 and not args.full and args.dump_outputs is None
    assert bench.parse(["--full", "--dump-outputs", "d"]).full
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
