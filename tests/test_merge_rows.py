"""The model of the pattern merge table (tests/merge_rows.py) against the torch sort of panfeed_amd.distributed, and the
cases against what they claim to reach.  No GPU: tests/test_gpu_merge_table.py runs the same cases through the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_rows as mr  # noqa: E402

from panfeed_amd.distributed import _first_per_digest, merge_pattern_tensors  # noqa: E402

UNPADDED = mr.unpadded_cases()
PADDED = mr.padded_cases()


def _i64(rows):
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64))


@pytest.mark.parametrize("name", list(UNPADDED))
def test_model_equals_the_torch_sort(name):
    rows, _ = UNPADDED[name]
    keep, nd = mr.marks(rows)
    t = _i64(rows)
    k_sort, n_sort = _first_per_digest(t)
    assert n_sort == nd and np.array_equal(k_sort.numpy(), keep)
    md5 = t[:, :2].contiguous().view(torch.uint8).view(-1, 16)
    k_one, n_one = merge_pattern_tensors(md5, t[:, 2].contiguous())
    assert n_one == nd and np.array_equal(k_one.numpy(), keep)


@pytest.mark.parametrize("name", list(PADDED))
def test_padded_model_equals_the_torch_sort_over_the_valid_rows(name):
    rows, counts, slot_rows = PADDED[name]
    keep, nd = mr.marks(rows, counts, slot_rows)
    # the selection merge_pattern_tensors makes of an all-gathered buffer before it sorts
    c = torch.tensor(counts, dtype=torch.int64)
    valid = (torch.arange(slot_rows)[None, :] < c[:, None]).reshape(-1)
    assert np.array_equal(valid.numpy(), mr.existing(len(rows), counts, slot_rows))
    k_sort, n_sort = _first_per_digest(_i64(rows)[valid])
    assert n_sort == nd and np.array_equal(k_sort.numpy(), keep[valid.numpy()])
    assert not keep[~valid.numpy()].any()


def test_model_by_hand():
    rows = np.array([[1, 2, 9], [1, 3, 4], [1, 2, 5], [2, 2, 5], [1, 2, 5], [1, 3, 6]], dtype=np.uint64)
    keep, nd = mr.marks(rows)
    assert nd == 3 and keep.tolist() == [False, True, True, True, True, False]
    keep, nd = mr.marks(rows, (1, 0, 2), 2)                    # rows 1, 2 and 3 are padding
    assert nd == 2 and keep.tolist() == [False, False, False, False, True, True]
    keep, nd = mr.marks(rows, (2, 0, 1), 2)                    # rows 2, 3 and 5 are padding: row 1 keeps its mark
    assert nd == 2 and keep.tolist() == [False, True, False, False, True, False]
    assert mr.marks(np.zeros((0, 3), dtype=np.uint64))[1] == 0


def test_capacity_rule_and_its_edges():
    assert [mr.capacity(n) for n in (1, 2, 511, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 1024, 2048, 2048, 4096]
    assert {f"sizes/{n}" for n in (1, 2, 511, 512, 513, 1024, 1025)} <= set(UNPADDED)
    for n in (1, 2, 511, 512, 513, 1024, 1025):
        rows, _ = UNPADDED[f"sizes/{n}"]
        assert len(rows) == n and mr.marks(rows)[0].all() and mr.marks(rows)[1] == n


@pytest.mark.parametrize("word,col", [("same_lo", 0), ("same_hi", 1)])
def test_same_word_cases_share_one_word(word, col):
    over, exact = UNPADDED[word + "/536"][0], UNPADDED[word + "/512"][0]
    assert len(exact) == 512 and mr.capacity(len(exact)) == 1024
    assert 512 < len(over) <= 560 and mr.capacity(len(over)) == 2048
    for rows in (over, exact):
        assert len(set(rows[:, col].tolist())) == 1                       # one distinct word ...
        assert len(set(rows[:, 1 - col].tolist())) == 512                 # ... under 512 digests
        assert mr.marks(rows)[1] == 512
    per_digest = np.unique(over[:, 1 - col], return_counts=True)[1]
    assert set(per_digest.tolist()) == {1, 2, 3}
    assert len(set(over[:, 2].tolist())) == len(over)
    if col == 0:
        # equal first words meet in the table whatever the slot function: some digest does not sit in its home slot
        taken, cap = mr.occupied_slots(exact)
        homes = {mr.home_slot(int(r[0]), int(r[1]), cap) for r in exact}
        assert len(taken) == 512 and len(homes) < 512


def test_wrap_chain_passes_slot_zero():
    rows, _ = UNPADDED["wrap"]
    taken, cap = mr.occupied_slots(rows)
    assert cap == 1024 and len(rows) == 80 and mr.marks(rows)[1] == 40
    homes = [mr.home_slot(int(r[0]), int(r[1]), cap) for r in rows]
    assert set(homes) == set(range(cap - 8, cap))
    assert taken == set(range(cap - 8, cap)) | set(range(32))             # over the end, through slot 0 and on
    assert np.unique(rows[:, :2], axis=0, return_counts=True)[1].tolist() == [2] * 40


@pytest.mark.parametrize("name,col", [("sentinel_lo", 0), ("sentinel_hi", 1)])
def test_sentinel_cases_hold_the_marker_and_its_neighbour(name, col):
    rows, _ = UNPADDED[name]
    words = set(rows[:, col].tolist())
    assert {mr.ONES, mr.ONES - 1} <= words
    if col == 0:
        assert 0 in words
        assert 0 in set(rows[:, 1].tolist())
        assert mr.ONES not in set(rows[:, 1].tolist()) and mr.ONES - 1 not in set(rows[:, 1].tolist())
    keep, nd = mr.marks(rows)
    assert nd * 3 == len(rows) and keep.sum() == nd
    # the smallest first_seen is the first, the second and the third copy in turn
    where = {int(i) // nd for i in np.flatnonzero(keep)}
    assert where == {0, 1, 2}


@pytest.mark.parametrize("name,at", [("one_digest/min_first", 0), ("one_digest/min_last", 4095), ("one_digest/min_middle", 2048)])
def test_one_digest_has_one_mark(name, at):
    rows, _ = UNPADDED[name]
    keep, nd = mr.marks(rows)
    assert len(rows) == 4096 and nd == 1 and np.flatnonzero(keep).tolist() == [at]
    assert len(set(rows[:, 2].tolist())) == 4096


def test_wave_shapes_layouts():
    eq, df = UNPADDED["wave_shapes/lanes_equal"][0], UNPADDED["wave_shapes/lanes_differ"][0]
    for rows in (eq, df):
        keep, nd = mr.marks(rows)
        assert len(rows) == 4096 and nd == 64 and keep.sum() == 64
    for w in range(64):
        assert len(np.unique(eq[64 * w:64 * w + 64, :2], axis=0)) == 1     # a wave's lanes hold one digest
        assert len(np.unique(df[64 * w:64 * w + 64, :2], axis=0)) == 64    # a wave's lanes hold 64 digests ...
        assert np.array_equal(df[64 * w:64 * w + 64, :2], df[:64, :2])     # ... lane l the same one in every wave
    lanes = {int(i) % 64 for i in np.flatnonzero(mr.marks(eq)[0])}
    assert len(lanes) > 16                                                 # the minima are not all in one lane


def test_ties_and_zero():
    rows, _ = UNPADDED["ties_and_zero"]
    keep, nd = mr.marks(rows)
    assert nd == 6
    assert keep.tolist() == [True, True, True, True, False, True, False, True, False, True, True, True, True]
    assert 0 in rows[:, 2].tolist() and mr.FS_LIMIT - 1 in rows[:, 2].tolist()


def test_padding_looks_like_real_rows():
    rows, counts, S = PADDED["padded/early_copies"]
    assert counts == (S, 0, 1, S - 1) and S == 300 and len(rows) == 4 * S
    live = mr.existing(len(rows), counts, S)
    least = {}
    for r in rows[live]:
        d = (int(r[0]), int(r[1]))
        least[d] = min(least.get(d, mr.ONES), int(r[2]))
    pad = rows[~live]
    assert all((int(r[0]), int(r[1])) in least and int(r[2]) < least[(int(r[0]), int(r[1]))] for r in pad)
    # taken for real, every one of them would take its digest's mark away
    assert len({(int(r[0]), int(r[1])) for r in pad}) > 200
    assert (PADDED["padded/all_ones"][0][~live] == mr.ONES).all()
    fresh = PADDED["padded/fresh"][0][~live]
    assert not any((int(r[0]), int(r[1])) in least for r in fresh)
    # the real rows: digests seen by two and by three ranks, the first sighting on either side
    keep, nd = mr.marks(rows, counts, S)
    assert nd == 300 + 149 and 0 < keep[:S].sum() < S and 0 < keep[3 * S:].sum() < S - 1
    for other in ("padded/all_ones", "padded/fresh"):
        assert np.array_equal(PADDED[other][0][live], rows[live])


def test_cases_stay_inside_the_stated_limits():
    for name, (rows, rng) in UNPADDED.items():
        assert rows.dtype == np.uint64 and rows.ndim == 2 and rows.shape[1] == 3 and 1 <= len(rows) <= 8192, name
        assert not mr.aliased(rows), name
        assert int(rows[:, 2].max()) < mr.FS_LIMIT, name
        assert rng[0] == (0, len(rows)) and (0, 0) in rng and (len(rows) - 1, 1) in rng, name
        assert all(f + c <= len(rows) for f, c in rng), name
    for name, (rows, counts, S) in PADDED.items():
        live = mr.existing(len(rows), counts, S)
        assert not mr.aliased(rows[live]), name
        assert int(rows[live][:, 2].max()) < mr.FS_LIMIT, name


def test_aliased_tells_the_pairs_the_kernels_cannot():
    h = 12345
    assert mr.aliased(np.array([[mr.ONES, h, 1], [mr.ONES - 1, h, 2]], dtype=np.uint64))
    assert mr.aliased(np.array([[h, mr.ONES, 1], [h, mr.ONES - 1, 2]], dtype=np.uint64))
    assert not mr.aliased(np.array([[mr.ONES, h, 1], [mr.ONES - 1, h + 1, 2], [mr.ONES, h, 3]], dtype=np.uint64))
