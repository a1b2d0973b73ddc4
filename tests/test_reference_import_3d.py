"""Import of a `3d_fullres` model folder written by the reference's trainer (cineflow.reference_models), host side: the 3-D plans
translation and its refusals, the 2-D / 3-D dispatch of the importer, the tensor-name / shape check against Generic_UNet3D, and the
host-side capability probe of the native 3-D convolution (cf_conv3d_f16s_ok: no launch, no GPU).

The fixture tree tests/golden/ref_model_folder_3d/ was written by the reference's own save_checkpoint (make_golden_refckpt3d.py)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEG3D = os.path.join(HERE, "golden", "ref_model_folder_3d")
FLOW = os.path.join(HERE, "golden", "ref_model_folder", "flow")
POOL, KERN = [[1, 2, 2], [2, 2, 2]], [[1, 3, 3], [3, 3, 3], [3, 3, 3]]


def _R():
    from cineflow import reference_models
    return reference_models


def _plans():
    return _R().load_reference_pickle(os.path.join(SEG3D, "plans.pkl"))


def _with_stage(plans, **kw):
    return dict(plans, plans_per_stage={0: dict(plans["plans_per_stage"][0], **kw)})


def _rewrite_checkpoint(path, edit):
    """load a reference checkpoint in full (the numpy globals admitted), change its state_dict, write it back in the same layout"""
    R = _R()
    with torch.serialization.safe_globals(R._numpy_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    edit(ck["state_dict"])
    torch.save(ck, path)


def test_plans_translation_of_the_3d_fixture():
    R = _R()
    plans = _plans()
    assert isinstance(plans["plans_per_stage"][0]["patch_size"], np.ndarray) and len(plans["plans_per_stage"][0]["patch_size"]) == 3
    p = R.plans_from_reference_3d(plans)
    assert p["num_classes"] == 4 and p["num_modalities"] == 1
    assert p["patch_size"] == [8, 32, 32] and p["mirror_axes"] == [0, 1, 2]
    assert p["seg_net"] == {"dim": 3, "base_num_features": 4, "num_pool": 2, "pool_op_kernel_sizes": POOL, "conv_kernel_sizes": KERN}
    assert p["preprocessor_name"] == "GenericPreprocessor" and p["stage"] == 0
    assert p["transpose_forward"] == [0, 1, 2] and p["transpose_backward"] == [0, 1, 2]
    assert p["normalization_schemes"] == {"0": "nonCT"} and p["use_mask_for_norm"] == {"0": False}
    assert p["plans_per_stage"]["0"]["current_spacing"] == [10.0, 1.5, 1.5]
    assert p["dataset_properties"]["intensityproperties"]["0"]["mean"] == 101.25
    assert "flow_net" not in p and "crop_size" not in p
    assert json.loads(json.dumps(p)) == p                                            # plain JSON values only


def test_the_2d_translation_still_refuses_the_3d_plans():
    with pytest.raises(NotImplementedError, match="patch_size"):
        _R().plans_from_reference(_plans())


def test_3d_refusals_name_their_key():
    R = _R()
    plans = _plans()
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):
        R.plans_from_reference_3d(_with_stage(plans, pool_op_kernel_sizes=[[1, 2, 2], [3, 2, 2]]))
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        R.plans_from_reference_3d(_with_stage(plans, conv_kernel_sizes=[[1, 3, 3], [3, 3, 3], [5, 3, 3]]))
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        R.plans_from_reference_3d(_with_stage(plans, conv_kernel_sizes=[[3, 1, 3], [3, 3, 3], [3, 3, 3]]))
    with pytest.raises(NotImplementedError, match="conv_per_stage"):
        R.plans_from_reference_3d(dict(plans, conv_per_stage=3))
    with pytest.raises(NotImplementedError, match="patch_size"):
        R.plans_from_reference_3d(_with_stage(plans, patch_size=np.array([64, 64])))


def test_several_stages_take_the_last_one_unless_told():
    R = _R()
    plans = _plans()
    low = dict(plans["plans_per_stage"][0], current_spacing=np.array([10.0, 3.0, 3.0]))
    two = dict(plans, plans_per_stage={0: low, 1: plans["plans_per_stage"][0]})
    p = R.plans_from_reference_3d(two)
    assert p["stage"] == 1 and p["plans_per_stage"]["1"]["current_spacing"] == [10.0, 1.5, 1.5]
    assert R.plans_from_reference_3d(two, stage=0)["stage"] == 0
    with pytest.raises(KeyError, match="stage"):
        R.plans_from_reference_3d(two, stage=2)


def test_import_picks_the_3d_translation_and_checks_against_generic_unet_3d(tmp_path):
    R = _R()
    from cineflow.models import Generic_UNet3D
    from cineflow.predict import CineTrainer
    out = str(tmp_path / "out")
    R.main(["-s", SEG3D, "-o", out])
    with open(os.path.join(out, "plans.json")) as f:
        plans = json.load(f)
    assert plans["seg_net"]["dim"] == 3 and plans["patch_size"] == [8, 32, 32] and "flow_net" not in plans
    trainer = CineTrainer(plans, torch.device("cpu"), model_folder=out)
    assert isinstance(trainer.seg_net, Generic_UNet3D) and trainer.flow_net is None and trainer.processor is None
    ck = torch.load(os.path.join(out, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    assert set(ck) == {"seg_state_dict"}
    shapes = trainer.seg_net.state_shapes()
    assert {k: tuple(v.shape) for k, v in ck["seg_state_dict"].items()} == shapes
    assert shapes["conv_blocks_context.0.blocks.0.conv.weight"] == (4, 1, 1, 3, 3)
    assert shapes["conv_blocks_context.1.blocks.0.conv.weight"] == (8, 4, 3, 3, 3)
    assert shapes["tu.0.weight"] == (16, 8, 2, 2, 2) and shapes["tu.1.weight"] == (8, 4, 1, 2, 2)


def test_a_3d_folder_with_a_flow_folder_is_refused(tmp_path):
    with pytest.raises(ValueError, match="flow path is 2-D"):
        _R().main(["-s", SEG3D, "-w", FLOW, "-o", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()


def test_plans_with_dim_3_and_a_flow_net_raise():
    from cineflow.predict import CineTrainer
    p = _R().plans_from_reference_3d(_plans())
    p["flow_net"] = {"variant": "video", "kwargs": {}}
    p["crop_size"] = 32
    with pytest.raises(ValueError, match="flow_net"):
        CineTrainer(p, torch.device("cpu"))


@pytest.mark.parametrize("what", ["renamed", "reshaped"])
def test_a_wrong_tensor_fails_the_import_loudly(tmp_path, what):
    R = _R()
    seg = str(tmp_path / "seg3d")
    shutil.copytree(SEG3D, seg)
    key = "module.conv_blocks_context.1.blocks.0.conv.weight"

    def edit(sd):
        assert key in sd
        if what == "renamed":
            sd["module.conv_blocks_context.1.blocks.0.convolution.weight"] = sd.pop(key)
        else:
            sd[key] = sd[key][:, :, :1].contiguous()                                # (8, 4, 1, 3, 3): a (1,3,3) kernel where the plans say (3,3,3)
    _rewrite_checkpoint(os.path.join(seg, "fold_0", "model_final_checkpoint.model"), edit)
    with pytest.raises(KeyError if what == "renamed" else ValueError, match="conv_blocks_context.1.blocks.0.conv"):
        R.import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_conv3d_probe_answers_on_the_host():
    """cf_conv3d_f16s_ok is host code: one accepted shape and the three kinds of decline the header names"""
    from cineflow import _lib, ops
    h = _lib.lib()
    # B, C1, C2, D, H, W, Cout, KD, KH, stride_d, stride_hw
    assert h.cf_conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, 3, 3, 1, 1) == 1
    assert h.cf_conv3d_f16s_ok(2, 64, 64, 10, 64, 56, 64, 1, 3, 2, 2) == 1
    assert h.cf_conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, 5, 5, 1, 1) == 0          # k = 5
    assert h.cf_conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, 3, 5, 1, 1) == 0
    assert h.cf_conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, 3, 3, 3, 1) == 0          # stride 3
    assert h.cf_conv3d_f16s_ok(1, 32, 0, 64, 512, 512, 32, 3, 3, 1, 1) == 0          # 32 x 64 x 512 x 512 x 4 B = 2 GiB per sample
    assert h.cf_conv3d_f16s_ok(1, 16, 0, 64, 512, 512, 32, 3, 3, 1, 1) == 0          # the OUTPUT sample is 2 GiB
    assert h.cf_conv3d_f16s_ok(4, 16, 0, 64, 512, 512, 16, 3, 3, 1, 1) == 1          # 1 GiB samples: the batch is cut inside the library
    with ops.conv_terms(1):
        assert h.cf_conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, 3, 3, 1, 1) == 0      # one-term mode: only the three-term product is built
        assert not ops.conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, (3, 3, 3), (1, 1, 1))
    assert ops.conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, (3, 3, 3), (1, 1, 1))
    assert not ops.conv3d_f16s_ok(1, 32, 0, 20, 256, 224, 32, (3, 3, 3), (1, 2, 1))  # unequal in-plane strides
    # the shapes the probe leaves to the composition (composition_is_faster (a), (b), (c); no geometry), each next to the nearest shape it
    # takes: the layer table of test_gpu_conv3d_layer_routes.py runs the declined side of these same tuples
    from _conv3d_layer_refs import PROBE_PAIRS
    assert len(PROBE_PAIRS) >= 8
    for what, declined, taken in PROBE_PAIRS:
        assert h.cf_conv3d_f16s_ok(*declined) == 0, (what, declined)
        assert h.cf_conv3d_f16s_ok(*taken) == 1, (what, taken)
