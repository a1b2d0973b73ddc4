"""Region-based model folders (nnUNetTrainerV2BraTSRegions*: sigmoid heads, regions_class_order) through the importer and CineTrainer,
on the CPU: the fixture the reference's own writers produced (tests/golden/ref_model_regions), the plans keys, every refusal, the two
BatchNorm softmax rows, and the restated 2-D window loop of tests/_region_refs.py against the oracle's.

On the parent commit every test here fails: the importer knows neither the trainers nor the flags (the fixture folder dies in
check_state_dict's shape report), CineTrainer ignores the keys, and SEG_VARIANTS lacks the two rows."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import _region_refs as RR
from cineflow import reference_models as R
from cineflow.trainer import CineTrainer, default_plans

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
BRATS = {"whole tumor": [1, 2, 3], "tumor core": [2, 3], "enhancing tumor": [3]}
REGION_TRAINERS = {
    "nnUNetTrainerV2BraTSRegions": None, "nnUNetTrainerV2BraTSRegions_Dice": None, "nnUNetTrainerV2BraTSRegions_DDP": None,
    "nnUNetTrainerV2BraTSRegions_DA3": None, "nnUNetTrainerV2BraTSRegions_DA3_BD": None,
    "nnUNetTrainerV2BraTSRegions_DA3_BN": "bn", "nnUNetTrainerV2BraTSRegions_DA3_BN_BD": "bn",
    "nnUNetTrainerV2BraTSRegions_DA4_BN": "bn", "nnUNetTrainerV2BraTSRegions_DA4_BN_BD": "bn",
}


def renamed(dim, dst, name):
    """the fixture folder with another trainer name in its .model.pkl"""
    RR.folder(dim, dst)
    p = os.path.join(dst, "fold_0", RR.CHK + ".model.pkl")
    info = R.load_reference_pickle(p)
    info["name"], info["class"] = name, "<class '%s'>" % name
    with open(p, "wb") as f:
        pickle.dump(info, f)
    return dst


def region_plans(dim=3):
    p = default_plans(32, flow_variant=None, seg_base=4, seg_pool=2)
    p["num_classes"] = 3
    if dim == 3:
        p.update(patch_size=[6, 24, 20], mirror_axes=[0, 1, 2])
        p["seg_net"].update(dim=3, pool_op_kernel_sizes=[[1, 2, 2], [2, 2, 2]], conv_kernel_sizes=[[1, 3, 3], [3, 3, 3], [3, 3, 3]])
    p["seg_net"].update(regions=dict(BRATS), regions_class_order=[1, 2, 3])
    return p


@pytest.mark.parametrize("dim", ["2d", "3d"])
def test_fixture_folder_imports_with_the_region_keys(dim, tmp_path):
    out = str(tmp_path / "out")
    plans = R.import_reference_model_folder(RR.folder(dim, str(tmp_path / "ref")), None, out)
    with open(os.path.join(out, "plans.json")) as f:
        written = json.load(f)
    for p in (plans, written):
        assert p["num_classes"] == 3 and p["num_modalities"] == 2 and "flow_net" not in p
        assert p["seg_net"]["regions"] == BRATS and list(p["seg_net"]["regions"]) == list(BRATS)         # JSON object order = channel order
        assert p["seg_net"]["regions_class_order"] == [1, 2, 3]
        assert "norm" not in p["seg_net"]
    t = CineTrainer(written, CPU)
    assert t.regions == BRATS and t.regions_class_order == [1, 2, 3]
    assert t.seg_net.inference_apply_nonlin == "sigmoid" and t.seg_net.num_classes == 3
    assert t._new_seg_net().inference_apply_nonlin == "sigmoid"                                           # every fold's network
    ck = torch.load(os.path.join(out, "fold_0", RR.CHK + ".model"), map_location="cpu", weights_only=True)
    head = max(k for k in ck["seg_state_dict"] if k.startswith("seg_outputs.") and k.endswith(".weight"))
    assert ck["seg_state_dict"][head].shape[0] == 3


def test_existing_folders_have_no_regions():
    t = CineTrainer(default_plans(32, flow_variant=None, seg_base=4, seg_pool=2), CPU)
    assert t.regions is None and t.regions_class_order is None and t.seg_net.inference_apply_nonlin == "softmax"
    from cineflow.models import FabiansUNet3D, Generic_UNet, Generic_UNet3D
    assert Generic_UNet.inference_apply_nonlin == Generic_UNet3D.inference_apply_nonlin == FabiansUNet3D.inference_apply_nonlin == "softmax"


def test_region_trainer_table():
    assert set(R.REGION_TRAINERS) == set(REGION_TRAINERS)
    for name, norm in REGION_TRAINERS.items():
        regions, order = R.seg_regions_spec(name)
        assert regions == BRATS and list(regions) == list(BRATS) and order == [1, 2, 3], name
        assert R.REGION_TRAINERS[name][1] == ({"norm": "bn"} if norm else {}), name
    assert R.seg_regions_spec("nnUNetTrainerV2") == (None, None)
    assert R.seg_regions_spec("x", "kits") == ({"kidney incl tumor": [1, 2], "tumor": [2]}, [1, 2])
    assert R.seg_regions_spec("x", '{"a": [1, 2], "b": [2]}', [4, 5]) == ({"a": [1, 2], "b": [2]}, [4, 5])
    with pytest.raises(ValueError, match="seg_regions_class_order"):
        R.seg_regions_spec("x", '{"a": [1]}')
    with pytest.raises(ValueError, match="seg_regions"):
        R.seg_regions_spec("x", None, [1, 2])
    with pytest.raises(ValueError, match="neither a region set"):
        R.seg_regions_spec("x", "brats2021")


def test_two_batchnorm_softmax_rows():
    """nnUNetTrainerV2BraTSRegions_BN is a plain softmax BatchNorm trainer despite its name; nnUNetTrainerV2_MMS likewise"""
    for name in ("nnUNetTrainerV2BraTSRegions_BN", "nnUNetTrainerV2_MMS"):
        assert R.SEG_VARIANTS[name] == {"norm": "bn"} and R.seg_variant_row(name) == {"norm": "bn"}
        assert name not in R.REGION_TRAINERS and R.seg_regions_spec(name) == (None, None)


def test_bn_softmax_row_imports_a_batchnorm_folder(tmp_path):
    import _variant_fixture as VF
    src = VF.folder("2d", "nnUNetTrainerV2_BN", str(tmp_path / "ref"))
    p = os.path.join(src, "fold_0", VF.CHK + ".model.pkl")
    info = R.load_reference_pickle(p)
    info["name"] = "nnUNetTrainerV2_MMS"
    with open(p, "wb") as f:
        pickle.dump(info, f)
    plans = R.import_reference_model_folder(src, None, str(tmp_path / "out"))
    assert plans["seg_net"]["norm"] == "bn" and plans["num_classes"] == 4 and "regions" not in plans["seg_net"]


def test_bn_region_trainer_takes_the_bn_row(tmp_path):
    """the fixture's InstanceNorm checkpoint under a _BN region trainer's name: the row asks for BatchNorm and says what is missing"""
    src = renamed("3d", str(tmp_path / "ref"), "nnUNetTrainerV2BraTSRegions_DA4_BN")
    with pytest.raises(ValueError, match=r"nnUNetTrainerV2BraTSRegions_DA4_BN builds BatchNorm.*running_mean"):
        R.import_reference_model_folder(src, None, str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))


def test_kits_on_the_three_channel_head_is_refused(tmp_path):
    src = RR.folder("3d", str(tmp_path / "ref"))
    with pytest.raises(ValueError, match=r"nnUNetTrainerV2BraTSRegions.*has 3 output channels, but there are 2 regions") as e:
        R.main(["-s", src, "-o", str(tmp_path / "out"), "--seg_regions", "kits"])
    assert "tensors have another shape" not in str(e.value)                   # not check_state_dict's generic report
    assert not os.path.exists(str(tmp_path / "out"))


def test_seg_regions_flags_serve_a_subclass_of_ones_own(tmp_path):
    src = renamed("2d", str(tmp_path / "ref"), "MyRegionTrainer")
    with pytest.raises(ValueError):                                            # a stock softmax import: 4 channels expected, 3 there
        R.import_reference_model_folder(src, None, str(tmp_path / "plain"))
    R.main(["-s", src, "-o", str(tmp_path / "out"), "--seg_regions", '{"outer": [1, 2, 3], "mid": [2, 3], "inner": [3]}',
            "--seg_regions_class_order", "3", "1", "2"])
    with open(os.path.join(str(tmp_path / "out"), "plans.json")) as f:
        sk = json.load(f)["seg_net"]
    assert list(sk["regions"]) == ["outer", "mid", "inner"] and sk["regions_class_order"] == [3, 1, 2]
    R.main(["-s", src, "-o", str(tmp_path / "out2"), "--seg_regions", "brats"])
    with open(os.path.join(str(tmp_path / "out2"), "plans.json")) as f:
        assert json.load(f)["seg_net"]["regions"] == BRATS


def test_flow_folder_next_to_a_region_folder_is_refused(tmp_path):
    src = RR.folder("2d", str(tmp_path / "ref"))
    flow = os.path.join(HERE, "golden", "ref_model_folder", "flow")
    with pytest.raises(ValueError, match=r"seg_net\.regions.*flow_net"):
        R.import_reference_model_folder(src, flow, str(tmp_path / "out"))
    with pytest.raises(ValueError, match=r"seg_net\.regions.*flow_net"):
        R.import_reference_model_folder(os.path.join(HERE, "golden", "ref_model_folder", "seg"), flow, str(tmp_path / "out"), seg_regions="brats")
    assert not os.path.exists(str(tmp_path / "out"))


# ------------------------------------------------------------------------------------------------ CineTrainer's refusals
def test_allowed_networks_build():
    assert CineTrainer(region_plans(3), CPU).seg_net.inference_apply_nonlin == "sigmoid"
    assert CineTrainer(region_plans(2), CPU).seg_net.inference_apply_nonlin == "sigmoid"
    p = region_plans(3)
    p["seg_net"]["norm"] = "bn"                                                 # a trainer-variant key next to the regions
    assert CineTrainer(p, CPU).regions == BRATS
    p = {"num_modalities": 1, "num_classes": 3, "patch_size": [8, 16, 16], "mirror_axes": [0, 1, 2], "transpose_forward": [0, 1, 2],
         "transpose_backward": [0, 1, 2],
         "seg_net": {"dim": 3, "arch": "resenc", "base_num_features": 4, "num_pool": 1, "pool_op_kernel_sizes": [[1, 1, 1], [2, 2, 2]],
                     "conv_kernel_sizes": [[3, 3, 3], [3, 3, 3]], "num_blocks_encoder": [1, 1], "num_blocks_decoder": [1],
                     "regions": dict(BRATS), "regions_class_order": [1, 2, 3]}}
    t = CineTrainer(p, CPU)
    assert t.seg_net.inference_apply_nonlin == "sigmoid" and t.regions_class_order == [1, 2, 3]


def test_regions_next_to_flow_net_are_refused():
    p = default_plans(64, seg_base=4, seg_pool=2, reduced=dict(in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32], d_model=32, bottleneck_heads=4,
                                                               dim_feedforward=64))
    p["num_classes"] = 3
    p["seg_net"].update(regions=dict(BRATS), regions_class_order=[1, 2, 3])
    with pytest.raises(ValueError, match=r"seg_net\.regions and flow_net"):
        CineTrainer(p, CPU)


def test_regions_next_to_mtl_are_refused():
    import _mtl_folder_fixture as MF
    p = MF.mtl_plans(MF.configs()[0])
    p["seg_net"].update(regions=dict(BRATS), regions_class_order=[1, 2, 3])
    with pytest.raises(ValueError, match=r"seg_net\.regions and seg_net\.arch == 'mtl'"):
        CineTrainer(p, CPU)


def test_regions_next_to_prev_stage_classes_are_refused():
    p = region_plans(3)
    p["seg_net"]["prev_stage_classes"] = [1, 2, 3]
    with pytest.raises(ValueError, match=r"seg_net\.regions and seg_net\.prev_stage_classes"):
        CineTrainer(p, CPU)


@pytest.mark.parametrize("change,message", [
    (lambda sk, p: sk.pop("regions_class_order"), r"seg_net\.regions without seg_net\.regions_class_order"),
    (lambda sk, p: sk.pop("regions"), r"seg_net\.regions_class_order without seg_net\.regions"),
    (lambda sk, p: sk.update(regions_class_order=[1, 2]), r"seg_net\.regions_class_order has 2 entries and seg_net\.regions has 3"),
    (lambda sk, p: p.update(num_classes=4), r"num_classes == 4 next to 3 seg_net\.regions"),
    (lambda sk, p: sk["regions"].update({"tumor core": []}), r"seg_net\.regions\['tumor core'\] is an empty region"),
    (lambda sk, p: sk["regions"].update({"tumor core": [2, 256]}), r"seg_net\.regions\['tumor core'\] holds a label outside 0\.\.255"),
    (lambda sk, p: sk.update(regions_class_order=[1, 2, 300]), r"seg_net\.regions_class_order must be a list of label values in 0\.\.255"),
    (lambda sk, p: sk.update(regions_class_order=[1, -2, 3]), r"seg_net\.regions_class_order must be a list of label values in 0\.\.255"),
])
def test_malformed_region_keys_are_refused(change, message):
    p = region_plans(3)
    change(p["seg_net"], p)
    with pytest.raises(ValueError, match=message):
        CineTrainer(p, CPU)


# ------------------------------------------------------------------------------------------------ the restated 2-D window loop
class _TinyNet(torch.nn.Module):
    num_classes = 3

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.a, self.b = torch.nn.Conv2d(2, 6, 3, padding=1), torch.nn.Conv2d(6, 3, 3, padding=1)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.4)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def test_restated_2d_loop_equals_the_oracles_bitwise_under_softmax():
    """the fixture's shapes: volume [2, 3, 56, 44], patch (48, 40), two tiles per axis, Gaussian weighting, both mirror axes"""
    from oracle import models as OM
    net = _TinyNet().eval()
    vol = torch.randn(2, 3, 56, 44, generator=torch.Generator().manual_seed(9)).numpy()
    kw = dict(step_size=0.5, use_gaussian=True, pad_border_mode="constant", pad_kwargs={"constant_values": 0})
    with torch.no_grad():
        seg_o, prob_o = OM.predict_3d_2dconv_tiled(net, vol, (48, 40), do_mirroring=True, mirror_axes=(0, 1), **kw)
        prob_r = RR.predict_3d_2dconv_tiled(lambda tile, mult: OM.mirror_and_predict_2d(net, tile, (0, 1), True, mult), 3, vol, (48, 40), **kw)
    assert prob_r.dtype == prob_o.dtype == np.float32 and prob_r.shape == prob_o.shape == (3, 3, 56, 44)
    assert np.array_equal(prob_r.view(np.uint32), prob_o.view(np.uint32))
    assert np.array_equal(prob_r.argmax(0), seg_o)
    # ... and smaller than the patch along one axis (padding, one tile along it), no Gaussian
    small = vol[:, :1, :40, :]
    kw["use_gaussian"] = False
    with torch.no_grad():
        _s, prob_o = OM.predict_3d_2dconv_tiled(net, small, (48, 40), do_mirroring=True, mirror_axes=(0, 1), **kw)
        prob_r = RR.predict_3d_2dconv_tiled(lambda tile, mult: OM.mirror_and_predict_2d(net, tile, (0, 1), True, mult), 3, small, (48, 40), **kw)
    assert np.array_equal(prob_r.view(np.uint32), prob_o.view(np.uint32))


def test_stored_probabilities_keep_the_side_of_the_threshold():
    """export.probabilities_as_stored: round-to-nearest fp16, except that for a region model a p in (0.5, 0.5 + 2^-12] goes up to the next
    fp16 -- `stored > 0.5` exactly where `p > 0.5`, at most one fp16 unit in the last place from p; softmax models are untouched"""
    from cineflow.export import probabilities_as_stored
    f32 = np.float32
    up = np.nextafter(np.float16(0.5), np.float16(1))
    p = np.array([0.5, np.nextafter(f32(0.5), f32(1)), 0.5 + 2.0 ** -12, np.nextafter(f32(0.5 + 2.0 ** -12), f32(1)), 0.5003, 0.5 - 1e-5,
                  np.nextafter(f32(0.5), f32(0)), 0.25, 0.0, 1.0, 0.7312], dtype=np.float32)
    plain = probabilities_as_stored(p)
    assert plain.dtype == np.float16 and np.array_equal(plain, p.astype(np.float16))
    stored = probabilities_as_stored(p, [1, 2, 3])
    assert stored.dtype == np.float16 and np.array_equal(stored > 0.5, p > 0.5)
    assert list(stored[:4]) == [np.float16(0.5), up, up, up] and np.array_equal(stored[4:], plain[4:])
    assert float(np.abs(stored.astype(np.float64) - p).max()) <= 2.0 ** -11
    for dim in ("2d", "3d"):                                                   # the fixtures: the stored member paints the label file's labels
        probs, seg = RR.expected(dim)["probs"].numpy(), RR.expected(dim)["seg"].numpy()
        assert not np.array_equal(RR.region_labels(probs.astype(np.float16), (1, 2, 3)), seg)
        assert np.array_equal(RR.region_labels(probabilities_as_stored(probs, (1, 2, 3)), (1, 2, 3)), seg)


def test_fixture_conditions_hold():
    """what the generator asserted, from the committed files alone: every region above 0.5 on 5-95 % of the voxels, the ambiguous share
    (|p - 0.5| <= bar_p in any channel) under the label tests' cap and equal to the recorded one, labels = the region rule on the probabilities"""
    idx = RR.index()
    assert idx["trainer"] == "nnUNetTrainerV2BraTSRegions" and idx["regions_class_order"] == [1, 2, 3] and idx["bar_p"] == RR.BAR_P
    for dim in ("2d", "3d"):
        e = RR.expected(dim)
        probs, seg = e["probs"].numpy(), e["seg"].numpy()
        assert list(e["volume"].shape) == idx[dim]["volume"] and probs.shape == (3,) + seg.shape
        above = [(probs[k] > 0.5).mean() for k in range(3)]
        assert all(0.05 <= a <= 0.95 for a in above) and np.allclose(above, idx[dim]["share_above_half"], atol=1e-12)
        share = RR.ambiguous(probs).mean()
        assert share <= RR.AMBIGUOUS_CAP and abs(share - idx[dim]["ambiguous_share"]) < 1e-12
        assert np.array_equal(seg, RR.region_labels(probs, (1, 2, 3)))
