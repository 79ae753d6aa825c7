"""The pattern merge table on the device (pf_merge_patterns / pf_merge_patterns_padded: merge_slot, merge_insert_kernel and
merge_lookup_kernel of csrc/pf_kernels.h, merge_impl of csrc/pf_api.hip) against the dict model of tests/merge_rows.py, on
rows no MD5 run gives: equal first or second words, chains over the table's end, the words next to the empty marker, waves
of one digest, padding that looks like real rows, and the context's scratch table at one size after another.  Every
comparison is exact equality; the model's two stated limits (first_seen < 2^63, the all-ones aliasing) bound the cases,
see tests/merge_rows.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_rows as mr  # noqa: E402

pytestmark = pytest.mark.gpu

UNPADDED = mr.unpadded_cases()
PADDED = mr.padded_cases()
POISON = 0xAA                # the marks are written over this: a byte the kernel left alone is neither 0 nor 1
GUARD = 64                   # bytes behind the marks that must stay poison


@pytest.fixture(scope="module")
def eng():
    from panfeed_amd.engine import Engine
    e = Engine(klength=21, max_strains=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    """the model's answers, made once"""
    out = {name: mr.marks(rows) for name, (rows, _) in UNPADDED.items()}
    out.update({name: mr.marks(*case) for name, case in PADDED.items()})
    return out


def _up(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()


def _marks_buffer(count):
    import torch
    return torch.full((count + GUARD,), POISON, dtype=torch.uint8, device="cuda")


def _read(buf, count, where):
    got = buf.cpu().numpy()
    assert (got[count:] == POISON).all(), where                      # nothing written behind this rank's marks
    return got[:count]


def _merge(eng, t, first, count, where):
    """(status, marks uint8 [count], n_global) of one pf_merge_patterns call; count 0 goes with a null `keep`"""
    import torch
    buf = _marks_buffer(count)
    ng = C.c_uint64(0xDEAD)
    torch.cuda.synchronize()                                         # the library runs on its own stream
    st = eng.L.pf_merge_patterns(eng.ctx, C.c_void_p(t.data_ptr()), t.shape[0], first, count,
                                 C.c_void_p(buf.data_ptr()) if count else None, C.byref(ng))
    return st, _read(buf, count, where), ng.value


def _check_unpadded(eng, model, name):
    from panfeed_amd.distributed import _first_per_digest
    rows, asked = UNPADDED[name]
    keep, nd = model[name]
    t = _up(rows)
    for first, count in asked:
        st, got, ng = _merge(eng, t, first, count, (name, first, count))
        assert st == 0 and ng == nd, (name, first, count, st, ng, nd)
        assert np.array_equal(got, keep[first:first + count].astype(np.uint8)), (name, first, count)
    again = [_merge(eng, t, 0, len(rows), name) for _ in range(2)]     # the whole range twice in a row
    assert again[0][0] == again[1][0] == 0 and again[0][2] == again[1][2] == nd, name
    assert np.array_equal(again[0][1], again[1][1]) and np.array_equal(again[0][1], keep.astype(np.uint8)), name
    # a third voice: torch's sort on the device, no engine
    k_sort, n_sort = _first_per_digest(t)
    assert n_sort == nd and np.array_equal(k_sort.cpu().numpy(), keep), name
    assert np.array_equal(t.cpu().numpy().view(np.uint64), rows), name     # the rows are read, never written


@pytest.mark.parametrize("name", [n for n in UNPADDED if n != "sentinel_hi"])
def test_marks_equal_the_model(eng, model, name):
    """every range of every case: n_global is the number of digests, the marks are the model's slice"""
    _check_unpadded(eng, model, name)


def test_sentinel_hi(eng, model):
    """second words equal to the empty marker and to the word below it, in a test function of its own: a second word is what
    a lane waits for when it finds a claimed entry, and the empty marker there reads as 'not yet published'.  merge_slot
    maps BOTH words off the marker before it probes (`if (hi == EMPTY64) hi = EMPTY64 - 1`, right after the same line
    for lo), so a published second word is never the marker and no lane waits for one that will not change."""
    _check_unpadded(eng, model, "sentinel_hi")


@pytest.mark.parametrize("name", list(PADDED))
def test_padding_changes_no_mark_and_no_count(eng, model, name):
    """pf_merge_patterns_padded once for every rank, the one with no rows and the one whose slot is full among them: copies
    of real digests with an earlier first_seen, all-ones rows and fresh digests behind the real rows are not there"""
    import torch
    rows, counts, S = PADDED[name]
    keep, nd = model[name]
    t = _up(rows)
    c = torch.tensor(counts, dtype=torch.int64, device="cuda")
    for rank, count in enumerate(counts):
        buf = _marks_buffer(count)
        ng = C.c_uint64(0xDEAD)
        torch.cuda.synchronize()
        st = eng.L.pf_merge_patterns_padded(eng.ctx, C.c_void_p(t.data_ptr()), len(counts), S, C.c_void_p(c.data_ptr()),
                                            rank, count, C.c_void_p(buf.data_ptr()) if count else None, C.byref(ng))
        got = _read(buf, count, (name, rank))
        want = keep[rank * S:rank * S + count].astype(np.uint8)
        wrong = np.flatnonzero(got != want)
        assert st == 0 and ng.value == nd and not len(wrong), \
            f"{name} rank {rank}: status {st}, n_global {ng.value} for {nd} digests, {len(wrong)} wrong marks {wrong[:8]}"


def test_scratch_table_reused_at_other_sizes(eng, model):
    """one context, 4 096 slots, then 1 024, then 2 048, then 4 096 again: each call answers as it does alone, and n_global
    never counts a digest of the call before"""
    for name in ("sizes/1025", "sizes/1", "same_lo/536", "sizes/1025"):
        rows, _ = UNPADDED[name]
        keep, nd = model[name]
        st, got, ng = _merge(eng, _up(rows), 0, len(rows), name)
        assert st == 0 and ng == nd, (name, st, ng, nd)
        assert np.array_equal(got, keep.astype(np.uint8)), name


def test_arguments(eng, model):
    import torch
    from panfeed_amd import _lib
    L = eng.L
    ng = C.c_uint64(0xDEAD)
    assert L.pf_merge_patterns(eng.ctx, None, 0, 0, 0, None, C.byref(ng)) == 0 and ng.value == 0      # no rows at all
    rows, _ = UNPADDED["sizes/513"]
    t = _up(rows)
    buf = _marks_buffer(len(rows))
    torch.cuda.synchronize()
    for first, count in ((0, 514), (513, 1), (1, 513), (514, 0)):
        assert L.pf_merge_patterns(eng.ctx, C.c_void_p(t.data_ptr()), 513, first, count, C.c_void_p(buf.data_ptr()),
                                   C.byref(ng)) == _lib.ERR_ARG, (first, count)
    prows, counts, S = PADDED["padded/fresh"]
    pt = _up(prows)
    c = torch.tensor(counts, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def padded(rank, count):
        return L.pf_merge_patterns_padded(eng.ctx, C.c_void_p(pt.data_ptr()), 4, S, C.c_void_p(c.data_ptr()), rank, count,
                                          C.c_void_p(buf.data_ptr()), C.byref(ng))
    assert padded(4, 1) == _lib.ERR_ARG                              # rank >= world
    assert padded(0, S + 1) == _lib.ERR_ARG                          # more rows than a slot holds
    assert (_read(buf, len(rows), "refused calls") == POISON).all()  # a refused call writes no mark
    # the context answers a good call afterwards
    keep, nd = model["sizes/513"]
    st, got, n = _merge(eng, t, 0, 513, "after the refused calls")
    assert st == 0 and n == nd == 513 and np.array_equal(got, keep.astype(np.uint8))
