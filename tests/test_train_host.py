"""Host side of cineflow.train / cineflow.train_net (no GPU): the learning-rate schedule, the deep-supervision weights, the loader's
batches, every refusal, and the presence of the training entry points in the header and the built library."""
import os
import re

import numpy as np
import pytest

import _train_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("cf_conv2d_wgrad_splits", "cf_conv2d_wgrad", "cf_conv2d_dgrad", "cf_norm_act_bwd", "cf_dc_ce_loss_blocks", "cf_dc_ce_loss",
               "cf_grad_norm", "cf_sgd_nesterov")


def test_poly_lr():
    from cineflow.train import poly_lr
    assert poly_lr(0, 1000, 1e-2) == 1e-2
    assert poly_lr(500, 1000, 1e-2) == pytest.approx(1e-2 * 0.5 ** 0.9, rel=1e-15)
    assert poly_lr(999, 1000, 1e-2) == pytest.approx(1e-2 * 1e-3 ** 0.9, rel=1e-12)
    assert poly_lr(1000, 1000, 1e-2) == 0.0


def test_deep_supervision_weights_and_scales():
    from cineflow.train_net import deep_supervision_scales, deep_supervision_weights
    assert np.allclose(deep_supervision_weights(3), [2 / 3, 1 / 3, 0], rtol=1e-15)
    w6 = deep_supervision_weights(6)
    assert w6[-1] == 0 and np.allclose(w6[:5], np.array([16, 8, 4, 2, 1]) / 31, rtol=1e-15) and w6.sum() == pytest.approx(1, rel=1e-15)
    assert deep_supervision_scales([[2, 2], [2, 2], [2, 1]]) == [[1, 1], [0.5, 0.5], [0.25, 0.25]]


def _loader(stage, batch, threads, seed=3):
    from cineflow.train import Loader2D, make_generators
    from cineflow.validate import load_dataset
    ds = load_dataset(stage)
    return Loader2D(ds, list(ds.keys()), R.TINY_PATCH, batch, make_generators(seed)[0], threads=threads)


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    return R.write_stage_folder(tmp_path_factory.mktemp("train_host"))[1]


@pytest.mark.parametrize("batch,forced", [(2, 1), (12, 4)])
def test_loader_batches_do_not_depend_on_the_thread_count(stage, batch, forced):
    a, b = _loader(stage, batch, 1), _loader(stage, batch, 8)
    try:
        for _ in range(4):
            x, y = next(a), next(b)
            assert x["plan"] == y["plan"]
            assert np.array_equal(x["data"], y["data"]) and np.array_equal(x["seg"], y["seg"])
            assert x["data"].shape == (batch, 1, 40, 48) and x["seg"].shape == (batch, 40, 48) and x["seg"].dtype == np.int32
            flags = [p[3] for p in x["plan"]]
            assert flags == [False] * (batch - forced) + [True] * forced, "the LAST batch - round(batch * 0.67) elements are forced"
            for (key, sl, (y0, x0), is_forced), seg in zip(x["plan"], x["seg"]):
                if is_forced:          # the crop is centred on a foreground voxel of the chosen slice (its lower corner clamped below only)
                    assert (seg > 0).any()
                    if y0 > min(0, -((40 - seg.shape[0]) // 2)) and x0 > 0:
                        assert seg[20, 24] > 0
    finally:
        a.close()
        b.close()


def test_loader_pads_data_with_zero_and_seg_with_minus_one_then_zero(stage):
    ld = _loader(stage, 2, 2)
    try:
        data, _props = ld.case("case_002")                       # 36 x 40: smaller than the 40 x 48 patch on both axes
        out, seg = ld.fill(("case_002", 1, (-2, -4), False))
        assert np.array_equal(out[0, 2:38, 4:44], data[0, 1]) and np.array_equal(seg[2:38, 4:44], data[1, 1].astype(np.int32))
        border = np.ones((40, 48), bool)
        border[2:38, 4:44] = False
        assert (out[0][border] == 0).all() and (seg[border] == 0).all() and seg.min() >= 0
        plan = [p for _ in range(6) for p in next(ld)["plan"] if p[0] == "case_002"]
        free = [p for p in plan if not p[3]]
        assert free and all(p[2] == (-2, -4) for p in free), "a random crop of a case smaller than the patch has one possible box: centred"
        assert all(p[2][0] >= -2 and p[2][1] >= -4 for p in plan), "a foreground-centred box is clamped from below only, as the reference's"
    finally:
        ld.close()


def test_loader_state_resumes_the_stream(stage):
    a = _loader(stage, 2, 4)
    try:
        next(a)
        state = a.state()
        want = [next(a)["plan"] for _ in range(3)]
        a.set_state(state)
        assert [next(a)["plan"] for _ in range(3)] == want
    finally:
        a.close()


def test_refusals():
    from cineflow.train_net import TrainNet, check_servable
    for kw, key in ((dict(norm="bn"), "norm"), (dict(norm="gn"), "norm"), (dict(nonlin="relu"), "nonlin"), (dict(nonlin="gelu"), "nonlin"),
                    (dict(nonlin_slope=0.2), "nonlin"), (dict(block_order="conv_nonlin_norm"), "block_order")):
        with pytest.raises(ValueError, match="seg_net." + key):
            TrainNet(1, 8, 4, 3, **kw)
    base = {"num_modalities": 1, "num_classes": 4, "seg_net": {"base_num_features": 8, "num_pool": 3}}
    check_servable(base)
    for extra, key in (({"dim": 3}, "dim"), ({"regions": [[1, 2], [2]]}, "regions"), ({"prev_stage_classes": [1, 2]}, "prev_stage_classes"),
                       ({"arch": "resenc"}, "arch"), ({"arch": "mtl"}, "arch"), ({"norm": "bn"}, "norm")):
        with pytest.raises(ValueError, match=key):
            check_servable(dict(base, seg_net=dict(base["seg_net"], **extra)))
    with pytest.raises(ValueError, match="flow_net"):
        check_servable(dict(base, flow_net={"variant": "video"}))
    with pytest.raises(ValueError, match="regions"):
        check_servable(dict(base, regions={"a": [1, 2]}))
    with pytest.raises(ValueError, match="pool_op_kernel_sizes"):
        TrainNet(1, 8, 4, 2, pool_op_kernel_sizes=[(2, 2), (4, 4)])


def test_batch_dice_false_is_refused_on_the_host(tmp_path):
    from cineflow.train import SegTrainer
    with pytest.raises(ValueError, match="batch_dice"):
        SegTrainer("p.pkl", str(tmp_path), str(tmp_path), 0, batch_dice=False)


def test_parameter_names_and_layouts_are_the_inference_networks():
    from cineflow.models import Generic_UNet
    from cineflow.train_net import TrainNet
    for kw in (dict(), dict(seg_output_bias=True), dict(num_conv_per_stage=3)):
        pool = [(2, 2), (2, 2), (2, 1)]
        a = TrainNet(2, 8, 4, 3, pool_op_kernel_sizes=pool, **kw).state_shapes()
        b = Generic_UNet(2, 8, 4, 3, pool_op_kernel_sizes=pool, **kw).state_shapes()
        assert {k: tuple(v) for k, v in a.items()} == {k: tuple(v) for k, v in b.items()}


def test_entry_points_are_declared_and_exported():
    from cineflow import _lib
    header = open(os.path.join(ROOT, "include", "cineflow.h")).read()
    h = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert h.cf_conv2d_wgrad_splits(16, 8, 3, 3, 1, 7, 9) == 1
    assert h.cf_conv2d_wgrad_splits(0, 8, 3, 3, 1, 7, 9) < 0
    # argument checks run on the host before any launch
    assert h.cf_conv2d_wgrad(None, 1, None, 0, None, None, None, None, 0, 1, 8, 8, 4, 3, 3, 1, None) == -1
    assert h.cf_conv2d_dgrad(None, None, None, 4, 0, 0, 4, 4, 1, 8, 8, 4, 5, 5, 1, 0, None) == -1
    assert h.cf_dc_ce_loss(None, None, None, None, None, None, None, 2, 17, 64, 1e-5, 1.0, None) == -1
