"""cf_ensemble_pairs (csrc/ensemble.hip) through cineflow.ops.ensemble_pairs on the device.

For every listed pair p = (i, j) three statements of one result are compared, all exactly (integers and bytes: there is no tolerance):
  * seg[p] == ops.ensemble_merge([m_i, m_j], ...)[0] byte for byte, and hist[p] == cf_label_confusion(seg[p], gt, K = 16) count for count;
  * both == this file's numpy statement of nnunet/evaluation/model_selection/ensemble.py merge: np.mean((a, b), 0), argmax(0) (or the
    regions_class_order overwrite loop), the bounding-box placement into zeros, and np.bincount of 16 * test + reference with one overflow
    bin for the voxels that hold a label >= 16 in either volume.
Outputs are pre-filled with a sentinel (0xAB bytes, -7 counts), so an element the kernel does not write shows.

Members are seeded values rounded to multiples of 1/16 (softmax-like over K; independent in [0, 1] for the region runs), so exact ties of
the two-member means are frequent and the first-index rule decides them.  The pair list holds every combination of the members plus a
reversed pair and a repeated one: two list entries served by one combination.  Shapes are the smallest that reach every path: X in
{7, 8, 19} (a tail only, one whole chunk, whole chunks and a tail), x0 in {0, 3} and a right margin of 0 or 5 (aligned and unaligned rows,
margin chunks present or not), a crop that is the whole volume, Z = 1, a NaN member, a ground truth with a label 16, a region order with a
label 20, and one volume of 4.5 M voxels whose chunks outnumber the threads of the largest grid, so the grid-stride loop takes a second
trip (asserted from the launch shape)."""
import functools
from itertools import combinations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIST_K = 16
DTYPES = {"fp16": np.float16, "fp32": np.float32}
ORDER = (1, 2, 3, 2, 1)


def seeded_members(M, K, crop, regions, seed):
    rng = np.random.default_rng(seed)
    if regions:
        p = rng.random((M, K) + tuple(crop))
    else:
        e = np.exp(1.5 * rng.standard_normal((M, K) + tuple(crop)))
        p = e / e.sum(1, keepdims=True)
    return (np.round(16 * p) / 16).astype(np.float16)


def seeded_gt(full, seed, top=4):
    return np.random.default_rng(seed + 1000).integers(0, top, size=full).astype(np.uint8)


def pair_list(M):
    pairs = list(combinations(range(M), 2))
    return pairs + [(1, 0), pairs[-1]]


def numpy_pair(a, b, full, lo, order):
    mean = np.mean((a, b), 0)
    assert mean.dtype == a.dtype
    if order is None:
        seg = mean.argmax(0)
    else:
        seg = np.zeros(mean.shape[1:])
        for i, c in enumerate(order):
            seg[mean[i] > 0.5] = c
    out = np.zeros(full, dtype=np.uint8)
    out[tuple(slice(s, s + n) for s, n in zip(lo, seg.shape))] = seg
    return out


def numpy_hist(seg, gt):
    t, r = seg.astype(np.int64).ravel(), gt.astype(np.int64).ravel()
    inside = (t < HIST_K) & (r < HIST_K)
    h = np.bincount(t[inside] * HIST_K + r[inside], minlength=HIST_K * HIST_K)
    return np.concatenate([h, [np.count_nonzero(~inside)]])


def device_pairs(dev, members, pairs, gt, lo, order):
    from cineflow import ops
    P = len(pairs)
    seg = torch.full((P,) + tuple(gt.shape), 0xAB, dtype=torch.uint8, device=dev)
    hist = torch.full((P, HIST_K * HIST_K + 1), -7, dtype=torch.int64, device=dev)
    got = ops.ensemble_pairs([torch.from_numpy(np.array(m)).to(dev) for m in members], pairs, torch.from_numpy(np.array(gt)).to(dev), lo,
                             regions_class_order=order, out=(seg, hist))
    assert got[0] is seg and got[1] is hist
    return seg, hist


def device_merge_and_confusion(dev, a, b, gt, lo, order):
    """the chained route: ops.ensemble_merge, then cf_label_confusion on its volume"""
    from cineflow import ops
    from cineflow._lib import check, lib
    seg, _ = ops.ensemble_merge([torch.from_numpy(np.array(a)).to(dev), torch.from_numpy(np.array(b)).to(dev)], tuple(gt.shape), lo,
                                regions_class_order=order)
    gt_t = torch.from_numpy(np.array(gt)).to(dev)
    hist = torch.full((HIST_K * HIST_K + 1,), -7, dtype=torch.int64, device=dev)
    check(lib().cf_label_confusion(seg.data_ptr(), gt_t.data_ptr(), seg.numel(), HIST_K, hist.data_ptr(), None), "cf_label_confusion")
    torch.cuda.synchronize()
    return seg.cpu().numpy(), hist.cpu().numpy()


def check_case(dev, members, gt, lo, order, chained=True):
    M = len(members)
    pairs = pair_list(M)
    seg, hist = device_pairs(dev, members, pairs, gt, lo, order)
    seg, hist = seg.cpu().numpy(), hist.cpu().numpy()
    for p, (i, j) in enumerate(pairs):
        want = numpy_pair(members[i], members[j], gt.shape, lo, order)
        assert np.array_equal(seg[p], want), "pair %d = (%d, %d): %d voxels differ from numpy" % (p, i, j, int((seg[p] != want).sum()))
        want_hist = numpy_hist(want, gt)
        assert np.array_equal(hist[p], want_hist), "pair %d = (%d, %d): counts differ from numpy in bins %s" % (
            p, i, j, np.flatnonzero(hist[p] != want_hist)[:8])
        assert int(hist[p].sum()) == gt.size
        if chained:
            seg_m, hist_m = device_merge_and_confusion(dev, members[i], members[j], gt, lo, order)
            assert np.array_equal(seg[p], seg_m) and np.array_equal(hist[p], hist_m), (p, i, j)
    return seg, hist


@functools.lru_cache(maxsize=None)
def main_inputs(M, dtype, regions):
    members = [m.astype(DTYPES[dtype]) for m in seeded_members(M, 5, (5, 13, 19), regions, seed=M)]
    gt = seeded_gt((7, 16, 27), seed=M)
    for a in members + [gt]:
        a.setflags(write=False)
    return members, gt


@pytest.mark.parametrize("regions", [False, True], ids=["argmax", "regions"])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_pairs_equal_merge_confusion_and_numpy(dev, M, dtype, regions):
    members, gt = main_inputs(M, dtype, regions)
    seg, hist = check_case(dev, members, gt, (1, 2, 3), ORDER if regions else None)
    assert len({seg[p].tobytes() for p in range(len(seg))}) >= (M * (M - 1)) // 2          # the pairs are not all one volume


def test_the_seeded_means_tie_exactly_in_many_voxels():
    """CPU only: the first-index rule is exercised"""
    members, _ = main_inputs(3, "fp16", False)
    for i, j in combinations(range(3), 2):
        mean = np.sort(np.mean((members[i], members[j]), 0).astype(np.float32), 0)
        assert (mean[-1] == mean[-2]).mean() >= 0.01


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_every_row_shape(dev, dtype):
    """X in {7, 8, 19} x x0 in {0, 3} x right margin in {0, 5}: tails, whole chunks, aligned and unaligned rows, with and without margin chunks"""
    n = 0
    for X in (7, 8, 19):
        for x0 in (0, 3):
            for right in (0, 5):
                members = [m.astype(DTYPES[dtype]) for m in seeded_members(3, 3, (2, 3, X), False, seed=100 + n)]
                gt = seeded_gt((3, 4, x0 + X + right), seed=100 + n)
                check_case(dev, members, gt, (1, 0, x0), None, chained=(X, x0, right) in ((19, 3, 5), (8, 0, 0)))
                n += 1


@pytest.mark.parametrize("regions", [False, True], ids=["argmax", "regions"])
def test_crop_equal_to_the_volume_and_one_slice(dev, regions):
    order = ORDER[:4] if regions else None
    members = list(seeded_members(4, 4, (1, 9, 24), regions, seed=7))
    check_case(dev, members, seeded_gt((1, 9, 24), seed=7), (0, 0, 0), order)             # Z = 1, the crop is the volume, every access aligned
    members = list(seeded_members(2, 4, (1, 5, 11), regions, seed=8).astype(np.float32))
    check_case(dev, members, seeded_gt((1, 5, 11), seed=8), (0, 0, 0), order)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_a_nan_counts_as_the_maximum(dev, dtype):
    members = [m.astype(DTYPES[dtype]) for m in seeded_members(3, 4, (2, 6, 19), False, seed=21)]
    rng = np.random.default_rng(22)
    hit = rng.random(members[1].shape) < 0.05
    members[1][hit] = np.nan
    members[2][:, 0, 0, :3] = np.nan                                                       # NaN in every class: the first one stays
    gt = seeded_gt((2, 8, 24), seed=21)
    seg, _ = check_case(dev, members, gt, (0, 1, 5), None)
    assert hit[1:].any() and (seg[0] > 0).any()


def test_labels_from_16_on_go_to_the_overflow_bin(dev):
    members = list(seeded_members(3, 4, (2, 6, 19), True, seed=31))
    gt = seeded_gt((3, 8, 27), seed=31)
    gt[1, 2, 3:9] = 16
    gt[2, 7, 26] = 255
    _, hist = check_case(dev, members, gt, (1, 1, 3), None)
    assert (hist[:, -1] == 7).all()
    _, hist = check_case(dev, members, seeded_gt((3, 8, 27), seed=32), (1, 1, 3), (1, 20, 3, 2))     # a label 20 on the test side
    assert (hist[:, -1] > 0).all()


def test_the_grid_stride_loop_takes_a_second_trip(dev):
    """4.5 M voxels: more 8-voxel chunks than the largest grid has threads (8 blocks of 256 per compute unit)"""
    full, crop, lo = (9, 500, 1003), (9, 500, 1000), (0, 0, 3)
    units = full[0] * full[1] * ((lo[2] + 7) // 8 + (crop[2] + 7) // 8)
    threads = (torch.cuda.get_device_properties(dev).multi_processor_count & ~7) * 8 * 256
    assert threads < units < 2 * threads, (units, threads)
    rng = np.random.default_rng(41)
    members = [(rng.integers(0, 17, size=(2,) + crop) / 16).astype(np.float16) for _ in range(2)]
    gt = seeded_gt(full, seed=41, top=2)
    seg, hist = device_pairs(dev, members, [(0, 1)], gt, lo, None)
    want = numpy_pair(members[0], members[1], full, lo, None)
    assert np.array_equal(seg[0].cpu().numpy(), want)
    assert np.array_equal(hist[0].cpu().numpy(), numpy_hist(want, gt))


def test_wrapper_refusals(dev):
    from cineflow import ops
    m = [torch.zeros(2, 1, 2, 8, dtype=torch.float16, device=dev) for _ in range(3)]
    gt = torch.zeros(1, 2, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="1 members"):
        ops.ensemble_pairs(m[:1], [(0, 1)], gt)
    with pytest.raises(ValueError, match=r"pair \(1, 1\)"):
        ops.ensemble_pairs(m, [(1, 1)], gt)
    with pytest.raises(ValueError, match=r"pair \(0, 3\)"):
        ops.ensemble_pairs(m, [(0, 3)], gt)
    with pytest.raises(ValueError, match="0 pairs"):
        ops.ensemble_pairs(m, [], gt)
    with pytest.raises(ValueError, match="do not fit"):
        ops.ensemble_pairs(m, [(0, 1)], gt, (0, 1, 0))
    with pytest.raises(ValueError, match="gt must be"):
        ops.ensemble_pairs(m, [(0, 1)], gt.to(torch.int32))
