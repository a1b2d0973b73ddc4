"""The sliding windows on a region-based network (sigmoid heads, labels by regions_class_order) against the reference's own outputs:
tests/golden/ref_model_regions (make_golden_regions.py) holds the folders nnUNetTrainerV2BraTSRegions wrote, a seeded case and the
reference's probabilities and labels on it -- in 3-D from its own predict_3D, in 2-D from its own mirror routine inside the tile loop
restated in tests/_region_refs.py.

Bars (tests/_region_refs.py).  Probabilities: bar_p = 1e-4 / 4 + 2e-6 = 2.7e-5 -- the logits bar of the import tests through
|sigmoid'| <= 1/4, plus the 1e-6 accumulate bar and the same again for the merge's division.  Labels: equal outside the voxels where a
reference probability lies within bar_p of 0.5 in any channel, which may be at most 0.5 % of the voxels (recorded: 0.027 % in 2-D,
0.093 % in 3-D).  Two folds holding the same weights against one fold: 1e-6.

Measured on the MI355X (pytest -s prints the figures): probabilities against the fixture 6.6e-7 (predict_cine_2Dconv_tiled), 7.7e-7
(predict_3D_2Dconv_tiled), 2.4e-7 (predict_3D_3Dconv_tiled); labels differ in 0 voxels in all three, ambiguous or not; two folds against
one 3.6e-7 in 2-D and 0 in 3-D."""
import numpy as np
import pytest
import torch

import _region_refs as RR

pytestmark = pytest.mark.gpu
ORDER = (1, 2, 3)


@pytest.fixture(scope="module")
def trainers(tmp_path_factory):
    """{dim: CineTrainer of the imported fixture folder, fold 0 loaded}"""
    from cineflow import reference_models as R
    from cineflow.predict import load_model_and_checkpoint_files
    out = {}
    for dim in ("2d", "3d"):
        base = tmp_path_factory.mktemp("regions" + dim)
        model = str(base / "model")
        R.import_reference_model_folder(RR.folder(dim, str(base / "ref")), None, model)
        trainer, params = load_model_and_checkpoint_files(model, [0])
        trainer.load_ensemble(params)
        assert trainer.regions_class_order == list(ORDER) and trainer.seg_net.inference_apply_nonlin == "sigmoid"
        out[dim] = (trainer, params)
    return out


def compare(name, seg, prob, exp):
    ref_p, ref_s = exp["probs"].numpy(), exp["seg"].numpy()
    assert prob.shape == ref_p.shape and prob.dtype == np.float32 and seg.shape == ref_s.shape and seg.dtype == np.uint8
    d = float(np.abs(prob.astype(np.float64) - ref_p).max())
    amb = RR.ambiguous(ref_p)
    differ = int((seg != ref_s).sum())
    differ_clear = int(((seg != ref_s) & ~amb).sum())
    print("  %s: probabilities max |diff| %.3e (bar %.2e); labels differ in %d voxels, %d of them unambiguous; ambiguous share %.4f %%"
          % (name, d, RR.BAR_P, differ, differ_clear, 100 * amb.mean()))
    assert d <= RR.BAR_P
    assert amb.mean() <= RR.AMBIGUOUS_CAP
    assert differ_clear == 0
    assert set(np.unique(seg)) <= {0, 1, 2, 3} and len(np.unique(seg)) >= 3


def same_run_to_run(name, seg_a, prob_a, seg_b, prob_b):
    """two runs of the 2-D network differ in the last bits (the fp64 statistics atomics of the fused norms): the
    probabilities are held to the 1e-6 of the two-fold check, the labels to equality outside the voxels within that of the threshold"""
    d = float(np.abs(prob_a.astype(np.float64) - prob_b).max())
    near = (np.abs(prob_a.astype(np.float64) - 0.5) <= 1e-6).any(axis=0)
    print("  %s: max |diff| %.3e (bar 1e-6), labels differ in %d voxels" % (name, d, int((seg_a != seg_b).sum())))
    assert d <= 1e-6 and not ((seg_a != seg_b) & ~near).any()


def test_cine_window_2d(dev, trainers):
    """predict_cine_2Dconv_tiled, volume [2, 3, 56, 44], patch (48, 40): two tiles per axis, Gaussian weights, both mirror axes"""
    from cineflow.inference import predict_3D_2Dconv_tiled, predict_cine_2Dconv_tiled
    print()
    trainer, _ = trainers["2d"]
    exp = RR.expected("2d")
    vol = exp["volume"].numpy()
    (seg, prob), = predict_cine_2Dconv_tiled([trainer.seg_net], [vol], (48, 40), regions_class_order=ORDER)
    compare("predict_cine_2Dconv_tiled", seg, prob, exp)
    # the labels are the region rule on the returned probabilities, bit for bit
    assert np.array_equal(seg, RR.region_labels(prob, ORDER))
    # the per-slice driver: the same probabilities through cf_tile_accumulate / cf_tile_finalize, the same rule
    seg1, prob1 = predict_3D_2Dconv_tiled(trainer.seg_net, vol, (48, 40), regions_class_order=ORDER)
    compare("predict_3D_2Dconv_tiled", seg1, prob1, exp)
    assert np.array_equal(seg1, RR.region_labels(prob1, ORDER))
    # without the order nothing changes: the arg-max of the same probabilities
    (seg0, prob0), = predict_cine_2Dconv_tiled([trainer.seg_net], [vol], (48, 40))
    assert float(np.abs(prob0.astype(np.float64) - prob).max()) <= 1e-6 and np.array_equal(seg0, prob0.argmax(0).astype(np.uint8))
    # the trainer hands its own order on
    seg_t, prob_t = trainer.predict_preprocessed_data_return_seg_and_softmax(vol)
    assert np.array_equal(seg_t, RR.region_labels(prob_t, ORDER))
    same_run_to_run("trainer, one volume vs predict_3D_2Dconv_tiled", seg_t, prob_t, seg1, prob1)
    (seg_v, prob_v), = trainer.predict_volumes_seg([vol])
    assert np.array_equal(seg_v, RR.region_labels(prob_v, ORDER))
    same_run_to_run("trainer, predict_volumes_seg vs predict_cine_2Dconv_tiled", seg_v, prob_v, seg, prob)


def test_window_3d(dev, trainers):
    """predict_3D_3Dconv_tiled, volume [2, 8, 28, 24], patch (6, 24, 20): several tiles in two axes, eight flips"""
    from cineflow.inference import predict_3D_3Dconv_tiled
    print()
    trainer, _ = trainers["3d"]
    exp = RR.expected("3d")
    vol = exp["volume"].numpy()
    seg, prob = predict_3D_3Dconv_tiled(trainer.seg_net, vol, (6, 24, 20), regions_class_order=ORDER)
    compare("predict_3D_3Dconv_tiled", seg, prob, exp)
    assert np.array_equal(seg, RR.region_labels(prob, ORDER))
    seg0, prob0 = predict_3D_3Dconv_tiled(trainer.seg_net, vol, (6, 24, 20))
    assert float(np.abs(prob0.astype(np.float64) - prob).max()) <= 1e-6 and np.array_equal(seg0, prob0.argmax(0).astype(np.uint8))
    seg_t, prob_t = trainer.predict_preprocessed_data_return_seg_and_softmax(vol)
    assert np.array_equal(seg_t, RR.region_labels(prob_t, ORDER))
    same_run_to_run("trainer vs predict_3D_3Dconv_tiled", seg_t, prob_t, seg, prob)


@pytest.mark.parametrize("dim", ["2d", "3d"])
def test_two_folds_of_the_same_weights_equal_one_fold(dev, trainers, dim):
    """the ensemble stays the weighted mean in one buffer, 1 / (flips x folds): the same fold twice gives one fold's probabilities
    within 1e-6, and the labels are the region rule on the ensemble's probabilities"""
    print()
    trainer, params = trainers[dim]
    vol = RR.expected(dim)["volume"].numpy()
    trainer.load_ensemble(params)
    _seg1, prob1 = trainer.predict_volumes_seg([vol])[0]
    try:
        trainer.load_ensemble([params[0], params[0]])
        assert len(trainer.seg_nets) == 2 and all(n.inference_apply_nonlin == "sigmoid" for n in trainer.seg_nets)
        seg2, prob2 = trainer.predict_volumes_seg([vol])[0]
    finally:
        trainer.load_ensemble(params)
    d = float(np.abs(prob2.astype(np.float64) - prob1).max())
    print("  %s: two folds vs one, max |diff| %.3e (bar 1e-6)" % (dim, d))
    assert d <= 1e-6
    assert np.array_equal(seg2, RR.region_labels(prob2, ORDER))
