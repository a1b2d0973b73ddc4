"""csrc/dataset.hip on the device, compared exactly with numpy: np.argwhere(key == value)[ranks], src[key > 0][ranks] and the counts.

The scan block is 256 voxels.  The volumes (3, 5, 67) = 1005, (9, 70, 66) = 41580 and (2, 1, 4099) = 8198 voxels cross 3, 162 and 32 full
blocks and end in a partial block of 237, 108 and 6 voxels: the issue's sizes, unchanged.  Ranks: first, last, the last match of every block
and the first of the next one, duplicates, unsorted.

(3, 151, 149) = 67497 voxels are 264 scan blocks: select_scan_kernel takes a second trip of 256 blocks and carries the first trip's sum
into it, from flat index 65536 on.  (9, 251, 247) = 557973 voxels are 2180 blocks: select_count_kernel's 2048 workgroups take a second
grid-stride trip from flat index 524288 on.  The ranks on both sides of each of those two indices are asserted to be among those tested."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCAN = 256
SHAPES = [(3, 5, 67), (9, 70, 66), (2, 1, 4099), (3, 151, 149), (9, 251, 247)]
TRIP_EDGES = [SCAN * 256, SCAN * 2048]                          # the scan's second 256-block trip, the count's second grid-stride trip


def _labels(shape, seed, nvalues=4):
    rng = np.random.default_rng(seed)
    return rng.integers(0, nvalues, size=shape).astype(np.float32)


def _edge_ranks(match_flat, rng):
    """ranks on both sides of every scan-block edge of a flat boolean match array, plus first, last, duplicates; shuffled"""
    total = int(match_flat.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    before = np.cumsum(match_flat)[SCAN - 1::SCAN]             # matches up to the end of every full block
    ranks = [0, total - 1, total // 2, total // 2]
    for b in before.tolist():
        ranks += [b - 1, b]
    ranks = np.array([r for r in ranks if 0 <= r < total], dtype=np.int64)
    for edge in TRIP_EDGES:                                     # the last match before a trip edge and the first at or after it
        b = int(match_flat[:edge].sum())
        assert edge >= match_flat.size or not 0 < b < total or {b - 1, b} <= set(ranks.tolist())
    ranks = np.concatenate([ranks, ranks[:3], rng.integers(0, total, size=17)])
    rng.shuffle(ranks)
    return ranks


@pytest.mark.parametrize("shape", SHAPES)
def test_select_coords_matches_argwhere(dev, shape):
    from cineflow import ops
    seg = _labels(shape, 5)
    assert seg.size // SCAN >= 3 and seg.size % SCAN != 0
    t = torch.from_numpy(seg).to(dev)
    index = ops.RankIndex(t, [1, 2, 3, 7])
    assert index.totals.tolist() == [int((seg == v).sum()) for v in (1, 2, 3, 7)]
    assert ops.label_counts(t, [3, 0]).tolist() == [int((seg == 3).sum()), int((seg == 0).sum())]
    rng = np.random.default_rng(11)
    for v in (1, 2, 3):
        ranks = _edge_ranks((seg == v).reshape(-1), rng)
        want = np.argwhere(seg == v)[ranks]
        got = ops.select_coords(t, v, ranks, index)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(ranks), 3)
        assert np.array_equal(got.cpu().numpy(), want), (shape, v)
        assert np.array_equal(ops.select_coords(t, v, ranks).cpu().numpy(), want)          # without a shared index
    # every rank of one value, in order
    allr = np.arange(int((seg == 2).sum()))
    assert np.array_equal(ops.select_coords(t, 2, allr, index).cpu().numpy(), np.argwhere(seg == 2))


def test_value_absent_from_a_middle_block_and_altogether(dev):
    from cineflow import ops
    seg = _labels((3, 5, 67), 6)
    flat = seg.reshape(-1)
    flat[SCAN:2 * SCAN][flat[SCAN:2 * SCAN] == 1] = 0           # block 1 holds no voxel of value 1
    flat[flat == 3] = 2                                         # value 3 is nowhere
    t = torch.from_numpy(seg).to(dev)
    index = ops.RankIndex(t, [1, 3])
    assert index.totals.tolist() == [int((seg == 1).sum()), 0]
    n0 = int((flat[:SCAN] == 1).sum())
    ranks = np.array([n0 - 1, n0, n0 + 1, 0, int(index.totals[0]) - 1], dtype=np.int64)     # n0 is the first match of block 2
    want = np.argwhere(seg == 1)[ranks]
    assert want[1][2] + 67 * want[1][1] + 335 * want[1][0] >= 2 * SCAN
    assert np.array_equal(ops.select_coords(t, 1, ranks, index).cpu().numpy(), want)
    empty = ops.select_coords(t, 3, np.zeros(0, np.int64), index)
    assert tuple(empty.shape) == (0, 3)
    with pytest.raises(IndexError):
        ops.select_coords(t, 3, [0], index)
    with pytest.raises(IndexError):
        ops.select_coords(t, 1, [int(index.totals[0])], index)


def test_k_zero_and_every_voxel_matching(dev):
    from cineflow import ops
    seg = np.full((2, 1, 4099), 5.0, np.float32)
    t = torch.from_numpy(seg).to(dev)
    index = ops.RankIndex(t, [5])
    assert index.totals.tolist() == [seg.size]
    assert tuple(ops.select_coords(t, 5, [], index).shape) == (0, 3)
    rng = np.random.default_rng(3)
    ranks = _edge_ranks(np.ones(seg.size, bool), rng)
    assert np.array_equal(ops.select_coords(t, 5, ranks, index).cpu().numpy(), np.argwhere(seg == 5)[ranks])
    allr = np.arange(seg.size)
    assert np.array_equal(ops.select_coords(t, 5, allr, index).cpu().numpy(), np.argwhere(seg == 5))


@pytest.mark.parametrize("shape", SHAPES)
def test_select_values_positive_predicate_and_stride(dev, shape):
    """src[key > 0][ranks], and the fingerprint's [::10] on a count that is no multiple of 10"""
    from cineflow import ops
    rng = np.random.default_rng(21)
    key = _labels(shape, 8, nvalues=3) - 1.0                    # -1, 0, 1: the predicate is > 0, not != 0
    key.reshape(-1)[7] = np.nan
    src = rng.normal(size=shape).astype(np.float32)
    total = int((key > 0).sum())
    if total % 10 == 0:
        key.reshape(-1)[np.flatnonzero(key.reshape(-1) > 0)[0]] = 0
        total -= 1
    assert total % 10 != 0
    k, s = torch.from_numpy(key).to(dev), torch.from_numpy(src).to(dev)
    index = ops.RankIndex(k)
    assert index.totals.tolist() == [total]
    stride = np.arange(0, total, 10, dtype=np.int64)
    got = ops.select_values(s, k, stride, index).cpu().numpy()
    want = src[key > 0][::10]
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    ranks = _edge_ranks((key > 0).reshape(-1), rng)
    assert ops.select_values(s, k, ranks).cpu().numpy().tobytes() == src[key > 0][ranks].tobytes()


def test_wrappers_reject_cpu_tensors():
    from cineflow import ops
    with pytest.raises(TypeError):
        ops.label_counts(torch.zeros(2, 3, 4), [1])
    with pytest.raises(TypeError):
        ops.select_coords(torch.zeros(2, 3, 4), 1, [0])
