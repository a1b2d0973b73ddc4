"""The importer's trainer-variant table (cineflow.reference_models.SEG_VARIANTS) and the plans keys it writes, on the CPU.

One row per trainer class of the reference's nnUNet_variants/architectural_variants directory (TRAINERS: the class names, which are what
`.model.pkl` holds).  Trainers with a fixture under tests/golden/ref_model_variants are imported from the folder the reference's own
writers produced; the others from a folder fabricated here in the same layout (a seeded state_dict of the network the row builds, a
plain pickle with the trainer's name), which is enough for what the importer reads.

On the parent commit the rows of nnUNetTrainerV2_ReLU, _GeLU, _Mish, _LReLU_slope_2en1, _GN, _ReLU_convReLUIN and _lReLU_convReLUIN fail
here because those folders import without a word and with none of the keys; _BN, _NoNormalization*, _3ConvPerStage*, _*biasInSegOutput
fail there in check_state_dict's shape report."""
import json
import os
import pickle

import pytest
import torch

import _variant_fixture as VF
from cineflow import reference_models as R
from cineflow.trainer import CineTrainer, default_plans
from cineflow.weights import seeded_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
V = "nnUNetTrainerV2_"
SEG_VARIANT_KEYS = ("norm", "norm_groups", "nonlin", "nonlin_slope", "conv_per_stage", "block_order", "seg_output_bias")
# class name -> the seg_net keys its folder must import to
EXPECT = {
    V + "ReLU": {"nonlin": "relu"},
    V + "GeLU": {"nonlin": "gelu"},
    V + "Mish": {"nonlin": "mish"},
    V + "LReLU_slope_2en1": {"nonlin": "lrelu", "nonlin_slope": 0.2},
    V + "GN": {"norm": "gn", "norm_groups": 8},
    V + "BN": {"norm": "bn"},
    V + "NoNormalization": {"norm": "none"},
    V + "NoNormalization_lr1en3": {"norm": "none"},
    V + "ReLU_convReLUIN": {"nonlin": "relu", "block_order": "conv_nonlin_norm"},
    V + "lReLU_convReLUIN": {"block_order": "conv_nonlin_norm"},
    V + "ReLU_biasInSegOutput": {"nonlin": "relu", "seg_output_bias": True},
    V + "lReLU_biasInSegOutput": {"seg_output_bias": True},
    V + "3ConvPerStage": {"conv_per_stage": 3},
    V + "3ConvPerStageSameFilters": {"conv_per_stage": 3},
    V + "allConv3x3": {},
    V + "noDeepSupervision": {},
    V + "softDeepSupervision": {},
}
# every class the directory defines: the rows above, FRN (refused by name) and the ResencUNet trainers (their own route, arch = 'resenc')
TRAINERS = sorted(EXPECT) + [V + "FRN", V + "ResencUNet", V + "ResencUNet_DA3", V + "ResencUNet_DA3_BN"]


def variant_keys(plans):
    return {k: v for k, v in plans["seg_net"].items() if k in SEG_VARIANT_KEYS}


def fabricate(dst, name, net_keys=None, base=4, dim="2d"):
    """a trainer's output folder at dst: the fixture's plans at width `base`, a seeded state_dict of the Generic_UNet that seg_net keys
    `net_keys` build, `.model.pkl` naming `name`"""
    plans = R.load_reference_pickle(os.path.join(VF.TREE, "plans_%s.pkl" % dim))
    plans["base_num_features"] = base
    os.makedirs(os.path.join(dst, "fold_0"))
    with open(os.path.join(dst, "plans.pkl"), "wb") as f:
        pickle.dump(plans, f)
    tp = (R.plans_from_reference if dim == "2d" else R.plans_from_reference_3d)(plans)
    tp["seg_net"].update(net_keys or {})
    if dim == "2d":
        tp["image_size"] = tp["patch_size"][0]
    sd = seeded_state_dict(CineTrainer(tp, torch.device("cpu")).seg_net.state_shapes(), seed=5)
    torch.save({"epoch": 3, "state_dict": sd}, os.path.join(dst, "fold_0", VF.CHK + ".model"))
    with open(os.path.join(dst, "fold_0", VF.CHK + ".model.pkl"), "wb") as f:
        pickle.dump({"init": ("plans.pkl", 0, "out", "nnUNet_preprocessed/Task031_x", True, None, True, True, False), "name": name,
                     "class": "<class '%s'>" % name, "plans": plans}, f)
    return dst


def test_the_table_has_a_row_for_every_trainer_of_the_directory():
    from cineflow import trainer
    assert tuple(trainer.SEG_VARIANT_KEYS) == SEG_VARIANT_KEYS
    for name in TRAINERS:
        assert name in R.SEG_VARIANTS or name == V + "FRN", name
    for name, keys in EXPECT.items():
        row = {k: v for k, v in R.SEG_VARIANTS[name].items() if k in SEG_VARIANT_KEYS}
        assert row == keys, name
    assert R.SEG_VARIANTS[V + "3ConvPerStage"]["base_num_features"] == 24
    assert R.SEG_VARIANTS[V + "allConv3x3"] == {"all_conv_3x3": True}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_imported_plans_hold_the_rows_keys(name, tmp_path):
    if name in VF.INDEX["2d"]:
        src = VF.folder("2d", name, str(tmp_path / "ref"))
    else:
        net_keys = dict(EXPECT[name], **({"base_num_features": 24} if name == V + "3ConvPerStage" else {}))
        src = fabricate(str(tmp_path / "ref"), name, net_keys)
    out = str(tmp_path / "out")
    plans = R.import_reference_model_folder(src, None, out)
    with open(os.path.join(out, "plans.json")) as f:
        written = json.load(f)
    assert variant_keys(plans) == variant_keys(written) == EXPECT[name]
    assert "flow_net" not in written and os.path.isfile(os.path.join(out, "fold_0", VF.CHK + ".model"))
    if name == V + "3ConvPerStage":
        assert written["seg_net"]["base_num_features"] == 24
    ck = torch.load(os.path.join(out, "fold_0", VF.CHK + ".model"), map_location="cpu", weights_only=True)
    assert not any(k.endswith("num_batches_tracked") for k in ck["seg_state_dict"])
    CineTrainer(written, torch.device("cpu"))                                 # the plans build


@pytest.mark.parametrize("name", sorted(VF.INDEX["3d"]))
def test_imported_3d_plans_hold_the_rows_keys(name, tmp_path):
    plans = R.import_reference_model_folder(VF.folder("3d", name, str(tmp_path / "ref")), None, str(tmp_path / "out"))
    assert plans["seg_net"]["dim"] == 3 and variant_keys(plans) == EXPECT[name]


def test_all_conv_3x3_overwrites_the_plans_kernels(tmp_path):
    src = fabricate(str(tmp_path / "ref"), V + "allConv3x3", {"conv_kernel_sizes": [[3, 3, 3]] * 3}, dim="3d")
    plans = R.import_reference_model_folder(src, None, str(tmp_path / "out"))
    assert plans["seg_net"]["conv_kernel_sizes"] == [[3, 3, 3]] * 3 and variant_keys(plans) == {}


def test_stock_folder_imports_without_any_of_the_keys(tmp_path):
    plans = R.import_reference_model_folder(os.path.join(HERE, "golden", "ref_model_folder", "seg"), None, str(tmp_path / "out"))
    assert variant_keys(plans) == {}
    with open(os.path.join(str(tmp_path / "out"), "plans.json")) as f:
        assert variant_keys(json.load(f)) == {}


def test_frn_is_refused_by_name(tmp_path):
    src = fabricate(str(tmp_path / "ref"), V + "FRN")
    with pytest.raises(NotImplementedError, match="nnUNetTrainerV2_FRN.*FRN3D"):
        R.import_reference_model_folder(src, None, str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))


@pytest.mark.parametrize("name,net_keys,message", [
    (V + "BN", {}, r"nnUNetTrainerV2_BN builds BatchNorm.*lacks conv_blocks_context\.0\.blocks\.0\.instnorm\.running_mean"),
    ("nnUNetTrainerV2", {"norm": "bn"}, r"trainer nnUNetTrainerV2 builds seg_net\.norm = 'in'.*conv_blocks_context\.0\.blocks\.0\.instnorm\.running_mean"),
    (V + "ReLU_biasInSegOutput", {}, r"nnUNetTrainerV2_ReLU_biasInSegOutput builds segmentation heads with a bias.*lacks seg_outputs\.0\.bias"),
    (V + "3ConvPerStage", {"base_num_features": 24}, r"nnUNetTrainerV2_3ConvPerStage builds 3 convolutions per stage.*first stage has 2: conv_blocks_context\.0\.blocks\.2"),
])
def test_table_and_checkpoint_must_agree(name, net_keys, message, tmp_path):
    src = fabricate(str(tmp_path / "ref"), name, net_keys)
    with pytest.raises(ValueError, match=message):
        R.import_reference_model_folder(src, None, str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))


def test_no_normalization_refuses_norm_tensors_and_3conv_checks_its_width(tmp_path):
    with pytest.raises(ValueError, match=r"nnUNetTrainerV2_NoNormalization builds no normalisation.*instnorm"):
        R.import_reference_model_folder(fabricate(str(tmp_path / "a"), V + "NoNormalization"), None, str(tmp_path / "out"))
    with pytest.raises(ValueError, match=r"nnUNetTrainerV2_3ConvPerStage sets base_num_features = 24.*has 4 output channels"):
        R.import_reference_model_folder(fabricate(str(tmp_path / "b"), V + "3ConvPerStage", {"conv_per_stage": 3}), None, str(tmp_path / "out"))


def test_seg_variant_flag_overrides_an_unknown_name(tmp_path):
    src = fabricate(str(tmp_path / "ref"), "MyOwnTrainer", {"norm": "bn"})
    with pytest.raises(ValueError, match="MyOwnTrainer.*running statistics"):
        R.import_reference_model_folder(src, None, str(tmp_path / "plain"))
    R.main(["-s", src, "-o", str(tmp_path / "out"), "--seg_variant", V + "BN"])
    with open(os.path.join(str(tmp_path / "out"), "plans.json")) as f:
        assert variant_keys(json.load(f)) == {"norm": "bn"}
    with pytest.raises(ValueError, match="no row of the trainer-variant table"):
        R.import_reference_model_folder(src, None, str(tmp_path / "bad"), seg_variant="nnUNetTrainerV2_Nope")


def _resenc_plans():
    return {"num_modalities": 1, "num_classes": 4, "patch_size": [8, 16, 16], "mirror_axes": [0, 1, 2], "transpose_forward": [0, 1, 2],
            "transpose_backward": [0, 1, 2],
            "seg_net": {"dim": 3, "arch": "resenc", "base_num_features": 4, "num_pool": 1, "pool_op_kernel_sizes": [[1, 1, 1], [2, 2, 2]],
                        "conv_kernel_sizes": [[3, 3, 3], [3, 3, 3]], "num_blocks_encoder": [1, 1], "num_blocks_decoder": [1]}}


@pytest.mark.parametrize("key,value", [("norm", "bn"), ("nonlin", "relu"), ("nonlin_slope", 0.2), ("norm_groups", 8), ("conv_per_stage", 3),
                                       ("block_order", "conv_nonlin_norm"), ("seg_output_bias", True)])
def test_cine_trainer_refuses_the_keys_next_to_another_architecture(key, value):
    import _mtl_folder_fixture as MF
    cpu = torch.device("cpu")
    p = _resenc_plans()
    CineTrainer(p, cpu)
    p["seg_net"][key] = value
    with pytest.raises(ValueError, match=r"seg_net\.%s and seg_net\.arch == 'resenc'" % key):
        CineTrainer(p, cpu)
    p = MF.mtl_plans(MF.configs()[0])
    p["seg_net"][key] = value
    with pytest.raises(ValueError, match=r"seg_net\.%s and seg_net\.arch == 'mtl'" % key):
        CineTrainer(p, cpu)
    p = default_plans(64, seg_base=4, seg_pool=2, reduced=dict(in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32], d_model=32, bottleneck_heads=4,
                                                               dim_feedforward=64))
    p["seg_net"][key] = value
    with pytest.raises(ValueError, match=r"seg_net\.%s and flow_net" % key):
        CineTrainer(p, cpu)


@pytest.mark.parametrize("key,value", [("norm", "frn"), ("nonlin", "swish"), ("block_order", "norm_conv_nonlin"), ("seg_output_bias", 1),
                                       ("norm_groups", 0), ("nonlin_slope", -0.1), ("conv_per_stage", 1)])
def test_cine_trainer_refuses_unknown_values(key, value):
    p = default_plans(64, flow_variant=None, seg_base=4, seg_pool=2)
    p["seg_net"][key] = value
    with pytest.raises(ValueError, match=r"seg_net\.%s" % key):
        CineTrainer(p, torch.device("cpu"))


def test_fixture_near_ties_stay_under_one_percent():
    """the share of voxels whose top-two reference logits lie within the logits bar, from the fixture alone (the GPU tests exclude them)"""
    for dim, name in VF.CASES:
        _x, logits = VF.expected(dim, name)
        share = float(VF.near_tie(logits, VF.BAR).double().mean())
        assert share <= 0.01 and abs(share - VF.INDEX[dim][name]["near_tie_share"]) < 1e-12, (dim, name, share)
    e = torch.load(os.path.join(VF.TREE, "e2e_bn_2d.pt"), map_location="cpu", weights_only=True)
    assert float(VF.near_tie(e["softmax"], VF.BAR, dim=0).double().mean()) <= 0.01
