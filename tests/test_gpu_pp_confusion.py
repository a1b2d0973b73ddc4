"""cf_pp_confusion / cf_cc_apply (csrc/cc_label.hip) against oracle.ops.remove_all_but_the_largest_connected_component applied in the
reference's sequence (connected_components.py:123-447): the foreground-joint filter on the raw image, the per-class filter on the raw
image, the per-class filter on the foreground-filtered image.  Counts are exact integers, images are compared voxel for voxel; with and
without size thresholds, and with z_skip.  Inputs: a seeded noise volume (hundreds of objects, many ties, odd sizes, several tiles) and the
seeded folders of tests/golden/postprocessing.  The oracle's images and counts are computed once per case on the CPU and shared."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocessing")
CLASSES = [1, 2, 3]
K = 4
SPACING = (1.25, 1.25, 8.0)
VPV = float(np.prod(SPACING, dtype=np.float64))
# thresholds in the units of kept_size (voxels x volume per voxel): the noise case's sizes are 1..~40 voxels, the folders' 27, 384 and more
THRESHOLDS = {"noise": {0: 6.5 * VPV, 1: 3.0 * VPV, 2: 2.0 * VPV, 3: 4.0 * VPV}, "D7": {0: 3900.0, 1: 300.0, 2: 1500.0, 3: 40.0 * VPV}}


@functools.lru_cache(maxsize=None)
def volumes(name):
    if name == "noise":
        rng = np.random.default_rng(11)
        shape = (5, 37, 43)
        pred = ((rng.random(shape) < 0.42) * rng.integers(1, 4, shape)).astype(np.uint8)
        pred[0:4, 0:8, 0:8] = 0                              # the largest class-3 object, behind a moat: not part of the largest foreground
        pred[0:3, 0:6, 0:6] = 3                              # object, so the per-class step keeps another one after the foreground step
        pred[-4:, -8:, -8:] = 0                              # and its twin: two largest class-3 objects of one size, a tie (both stay)
        pred[-3:, -6:, -6:] = 3
        gt = np.where(rng.random(shape) < 0.8, pred, rng.integers(0, 4, shape)).astype(np.uint8)
    else:
        fx = np.load(os.path.join(GOLDEN, name[0] + ".npz"))
        pred, gt = fx["pred"][int(name[1:])], fx["gt"][int(name[1:])]
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def oracle_mv(min_valid):
    return None if min_valid is None else {tuple(CLASSES): min_valid[0], 1: min_valid[1], 2: min_valid[2], 3: min_valid[3]}


@functools.lru_cache(maxsize=None)
def oracle_variants(name, thresholds):
    """the four images of the reference's sequence"""
    from oracle import ops as OO
    pred, _ = volumes(name)
    mv = oracle_mv(THRESHOLDS[name] if thresholds else None)
    fg, _, _ = OO.remove_all_but_the_largest_connected_component(pred.copy(), [tuple(CLASSES)], VPV, mv)
    per_raw, _, _ = OO.remove_all_but_the_largest_connected_component(pred.copy(), CLASSES, VPV, mv)
    per_fg, _, _ = OO.remove_all_but_the_largest_connected_component(fg.copy(), CLASSES, VPV, mv)
    out = (np.array(pred), fg, per_raw, per_fg)
    for a in out:
        a.setflags(write=False)
    return out


def oracle_counts(name, thresholds, z_skip):
    _, gt = volumes(name)
    out = np.zeros((4, K, 3), np.int64)
    for v, img in enumerate(oracle_variants(name, thresholds)):
        for c in range(K):
            t, r = (img == c)[z_skip[c]:], (gt == c)[z_skip[c]:]
            out[v, c] = [(t & r).sum(), (t & ~r).sum(), (~t & r).sum()]
    return out


def device_case(dev, name):
    from cineflow.evaluation import Loaded
    from cineflow.postprocessing import _Case
    pred, gt = volumes(name)
    props = {"itk_spacing": SPACING}
    assert torch.device(dev).type == "cuda"
    return _Case(Loaded("p", np.array(pred), props), Loaded("g", np.array(gt), props), CLASSES, K, False)


NAMES = ("noise", "D7")


def test_the_inputs_exercise_every_rule():
    """CPU only: every variant differs from every other, the thresholds spare objects, and a tie with the largest object exists."""
    from scipy.ndimage import label
    for name in NAMES:
        plain, thr = oracle_variants(name, False), oracle_variants(name, True)
        for a in range(4):
            for b in range(a + 1, 4 if name == "noise" else 1):            # (the folders' false objects are far from the heart: there the
                assert (plain[a] != plain[b]).any(), (name, a, b)          # foreground and the per-class filter may remove the same voxels)
        assert all((p != plain[0]).any() for p in plain[1:]), name
        assert any((p != t).any() for p, t in zip(plain[1:], thr[1:])), name
        assert all((t != plain[0]).any() for t in thr[1:]), name
    pred, _ = volumes("noise")
    ties = 0
    for c in CLASSES:
        sizes = np.bincount(label(pred == c)[0].reshape(-1))[1:]
        ties += int((sizes == sizes.max()).sum() > 1)
    print("classes of the noise volume whose largest size is shared:", ties)
    assert ties >= 1


@pytest.mark.parametrize("z_skip", [(0, 0, 0, 0), (0, 2, 0, 1)], ids=["all_slices", "z_skip"])
@pytest.mark.parametrize("thresholds", [False, True], ids=["always", "thresholds"])
@pytest.mark.parametrize("name", NAMES)
def test_counts_of_all_four_variants_equal_the_oracle(dev, name, thresholds, z_skip):
    from cineflow import ops
    case = device_case(dev, name)
    mv = THRESHOLDS[name] if thresholds else None
    got, _, _, _ = case.judge(mv)
    if any(z_skip):
        got = ops.pp_confusion(case.pred, case.gt, K, case.labels_fg, case.counts_fg, case.max_fg, case.labels_cls, case.counts_cls, case.max_cls,
                               case.max_cls_alive, VPV, mv, z_skip=dict(enumerate(z_skip))).cpu().numpy()
    want = oracle_counts(name, thresholds, z_skip)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), "counts differ at (variant, class, tp/fp/fn) %s" % np.argwhere(got != want).tolist()


@pytest.mark.parametrize("thresholds", [False, True], ids=["always", "thresholds"])
@pytest.mark.parametrize("name", NAMES)
def test_apply_equals_the_oracle_voxel_for_voxel(dev, name, thresholds):
    from oracle import ops as OO
    case = device_case(dev, name)
    mv = THRESHOLDS[name] if thresholds else None
    _, fg_max, raw_max, alive_max = case.judge(mv)
    raw, fg, per_raw, per_fg = oracle_variants(name, thresholds)
    assert np.array_equal(case.filtered(True, [], mv).cpu().numpy(), fg)
    assert np.array_equal(case.filtered(False, CLASSES, mv).cpu().numpy(), per_raw)
    assert np.array_equal(case.filtered(True, CLASSES, mv).cpu().numpy(), per_fg)
    assert np.array_equal(case.filtered(False, [], mv).cpu().numpy(), raw)
    for do_fg, single in ((True, [2]), (False, [1, 3])):
        src = fg.copy() if do_fg else raw.copy()
        want, _, _ = OO.remove_all_but_the_largest_connected_component(src, single, VPV, oracle_mv(mv))
        assert np.array_equal(case.filtered(do_fg, single, mv).cpu().numpy(), want), (do_fg, single)
    # the maxima the host gathers kept_size from: largest object of the raw image, per class before and after the foreground step
    _, _, kept_fg = OO.remove_all_but_the_largest_connected_component(raw.copy(), [tuple(CLASSES)], VPV)
    _, _, kept_raw = OO.remove_all_but_the_largest_connected_component(raw.copy(), CLASSES, VPV)
    _, _, kept_alive = OO.remove_all_but_the_largest_connected_component(fg.copy(), CLASSES, VPV)
    assert fg_max * VPV == kept_fg[tuple(CLASSES)]
    for c in CLASSES:
        assert raw_max[c] * VPV == kept_raw[c] and alive_max[c] * VPV == (kept_alive[c] or 0.0), c


def test_labels_at_and_above_k_pass_through_unscored(dev):
    """a prediction label outside the class list is neither filtered nor counted; a ground-truth label >= K is scored nowhere"""
    from cineflow.evaluation import Loaded
    from cineflow.postprocessing import _Case
    pred, gt = (np.array(a) for a in volumes("noise"))
    pred[0, :3, :3] = 9
    gt[1, :3, :3] = 200
    props = {"itk_spacing": SPACING}
    case = _Case(Loaded("p", pred, props), Loaded("g", gt, props), CLASSES, K, False)
    got, _, _, _ = case.judge(None)
    want = np.zeros((K, 3), np.int64)
    for c in range(K):
        t, r = pred == c, gt == c
        want[c] = [(t & r).sum(), (t & ~r).sum(), (~t & r).sum()]
    assert np.array_equal(got[0], want)
    out = case.filtered(True, CLASSES, None).cpu().numpy()
    assert (out[0, :3, :3] == 9).all()
