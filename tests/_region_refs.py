"""References for the region-based route (sigmoid heads, labels painted in regions_class_order), on the CPU.

`predict_3d_2dconv_tiled` restates the 2-D sliding window of SegmentationNetwork._internal_predict_3D_2Dconv_tiled /
_internal_predict_2D_2Dconv_tiled (neural_network.py:814-857, :623-769) AROUND a per-tile routine the caller supplies: the reference's own
loop passes its mirror routine a `normalize` argument that routine does not take (:718 / :573) and cannot run, and oracle.models' loop
hard-codes the softmax.  tests/golden/make_golden_regions.py hands it the reference's own _internal_maybe_mirror_and_pred_2D under the sigmoid;
tests/test_reference_import_regions.py shows that around oracle.models.mirror_and_predict_2d (softmax) it equals
oracle.models.predict_3d_2dconv_tiled bit for bit.  So the loop is a restatement, not pinned against a run of the reference's loop.

The bars of the region tests are here too, with the fixture tree's loader."""
import json
import os
import shutil

import numpy as np
import torch

from oracle import ops as OO

TREE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_model_regions")
CHK = "model_final_checkpoint"

LOGITS_BAR = 1e-4                      # tests/_variant_fixture.BAR: what the import tests hold the same kind of network's logits to
# |sigmoid'| <= 1/4 carries the logits bar into the probabilities; 1e-6 is the accumulate bar of the softmax twin (tests/test_gpu_ops.py),
# and the merge's division by the summed Gaussian weights is given the same again
BAR_P = LOGITS_BAR / 4 + 2e-6
AMBIGUOUS_CAP = 0.005                  # label comparisons may leave out at most this share of the voxels


def region_labels(probs, order):
    """probs [K, ...] -> labels: 0, then order[i] where probs[i] > 0.5, a later region overwriting an earlier one"""
    probs = np.asarray(probs)
    seg = np.zeros(probs.shape[1:], dtype=np.uint8)
    for i, c in enumerate(order):
        seg[probs[i] > 0.5] = c
    return seg


def ambiguous(probs_ref, bar=BAR_P):
    """bool mask over the voxels: some channel of the reference probabilities [K, ...] lies within `bar` of the 0.5 threshold"""
    return (np.abs(np.asarray(probs_ref, dtype=np.float64) - 0.5) <= bar).any(axis=0)


def predict_2d_tiled(tile_fn, num_classes, x, patch_size, step_size=0.5, use_gaussian=True, pad_border_mode="constant", pad_kwargs=None):
    """x: numpy [C,X,Y] -> probabilities [K,X,Y].  tile_fn(tile [1,C,ph,pw] tensor, mult [ph,pw] tensor or None) -> [1,K,ph,pw] tensor: the
    flip-averaged probabilities of one tile, already times `mult` (what _internal_maybe_mirror_and_pred_2D returns)."""
    patch_size = tuple(patch_size)
    data, slicer = OO.pad_nd_image(x, patch_size, pad_border_mode, pad_kwargs, True, None)
    steps = OO.compute_steps_for_sliding_window(patch_size, data.shape[1:], step_size)
    if use_gaussian and len(steps[0]) * len(steps[1]) > 1:
        add = OO.get_gaussian(patch_size, sigma_scale=1.0 / 8)
        mult = torch.from_numpy(add)
    else:
        add, mult = np.ones(patch_size, dtype=np.float32), None
    agg = np.zeros([num_classes] + list(data.shape[1:]), dtype=np.float32)
    cnt = np.zeros([num_classes] + list(data.shape[1:]), dtype=np.float32)
    for lx in steps[0]:
        for ly in steps[1]:
            tile = torch.from_numpy(np.ascontiguousarray(data[None, :, lx:lx + patch_size[0], ly:ly + patch_size[1]]))
            pred = tile_fn(tile, mult)[0].numpy()
            agg[:, lx:lx + patch_size[0], ly:ly + patch_size[1]] += pred
            cnt[:, lx:lx + patch_size[0], ly:ly + patch_size[1]] += add
    sl = tuple([slice(0, agg.shape[i]) for i in range(len(agg.shape) - (len(slicer) - 1))] + slicer[1:])
    return agg[sl] / cnt[sl]


def predict_3d_2dconv_tiled(tile_fn, num_classes, x, patch_size, **kw):
    """x: numpy [C,Z,X,Y] -> probabilities [K,Z,X,Y], slice by slice"""
    return np.stack([predict_2d_tiled(tile_fn, num_classes, x[:, z], patch_size, **kw) for z in range(x.shape[1])], axis=1)


# ------------------------------------------------------------------------------------------------ the fixture tree
def index():
    with open(os.path.join(TREE, "index.json")) as f:
        return json.load(f)


def folder(dim, dst):
    """the region trainer's output folder of dimension '2d' / '3d' at `dst` (created); returns dst"""
    os.makedirs(os.path.join(dst, "fold_0"))
    shutil.copy(os.path.join(TREE, "plans_%s.pkl" % dim), os.path.join(dst, "plans.pkl"))
    for ext in (".model", ".model.pkl"):
        shutil.copy(os.path.join(TREE, dim, CHK + ext), os.path.join(dst, "fold_0", CHK + ext))
    return dst


def expected(dim):
    """{'raw' [C,Z,Y,X], 'volume' [C,Z,Y,X], 'probs' [K,Z,Y,X], 'seg' [Z,Y,X]}: the seeded case as its files hold it, the same after the
    plans' preprocessing, and the reference's sliding-window probabilities and labels on that"""
    return torch.load(os.path.join(TREE, dim, "expected.pt"), map_location="cpu", weights_only=True)
