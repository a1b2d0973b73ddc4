"""Import of model folders written by the reference's trainers (cineflow.reference_models), host side: safe readers, plans translation,
the task-number rule, and the tensor-name / shape check against the networks the new plans build (constructed without a device).

The fixture tree tests/golden/ref_model_folder/ was written by the reference's own save_checkpoint (make_golden_refckpt.py)."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.join(HERE, "golden", "ref_model_folder")
SEG = os.path.join(TREE, "seg")
FLOW = os.path.join(TREE, "flow")
SEG_CK = os.path.join(SEG, "fold_0", "model_final_checkpoint.model")
FLOW_CK = os.path.join(FLOW, "Task031_x", "fold_0", "model_final_checkpoint.model")


def _R():
    from cineflow import reference_models
    return reference_models


def _copy_tree(tmp_path):
    dst = str(tmp_path / "ref")
    shutil.copytree(TREE, dst)
    return os.path.join(dst, "seg"), os.path.join(dst, "flow")


def _rewrite_checkpoint(path, edit):
    """load a reference checkpoint in full (the numpy globals admitted), change its state_dict, write it back in the same layout"""
    R = _R()
    with torch.serialization.safe_globals(R._numpy_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    edit(ck["state_dict"])
    torch.save(ck, path)


def test_plans_translation_of_the_fixture():
    R = _R()
    plans = R.load_reference_pickle(os.path.join(SEG, "plans.pkl"))
    assert isinstance(plans["plans_per_stage"][0]["patch_size"], np.ndarray)         # the planner's numpy values came through
    p = R.plans_from_reference(plans)
    assert p["num_classes"] == 4 and p["num_modalities"] == 1
    assert p["patch_size"] == [64, 64]
    assert p["seg_net"] == {"base_num_features": 8, "num_pool": 3, "pool_op_kernel_sizes": [[2, 2], [2, 2], [2, 2]]}
    assert p["transpose_forward"] == [0, 1, 2] and p["transpose_backward"] == [0, 1, 2]
    assert p["normalization_schemes"] == {"0": "nonCT"} and p["use_mask_for_norm"] == {"0": False}
    assert p["mirror_axes"] == [0, 1] and p["preprocessor_name"] == "PreprocessorFor2D" and p["stage"] == 0
    assert p["plans_per_stage"]["0"]["current_spacing"] == [8.0, 1.5, 1.5]
    assert p["dataset_properties"]["intensityproperties"]["0"]["mean"] == 101.25
    assert json.loads(json.dumps(p)) == p                                            # plain JSON values only


@pytest.mark.parametrize("task,successive,expected", [
    ("Task031_x", False, (128, 224, 7)), ("Task035_Lib", False, (128, 224, 7)), ("Task039_y", False, (192, 224, 7)),
    ("Task027_ACDC", False, (192, 384, 8)), ("Task031_x", True, (128, 224, 7)), ("Task039_y", True, (192, 384, 8)),
])
def test_task_number_rule(task, successive, expected):
    assert _R().crop_and_image_size(task, successive) == expected


def test_module_prefix_is_stripped():
    R = _R()
    ck = R.load_reference_checkpoint(SEG_CK)
    assert ck["state_dict"] and not any(k.startswith("module.") for k in ck["state_dict"])
    assert R.strip_module_prefix({"module.a": 1, "b": 2}) == {"a": 1, "b": 2}
    # network_trainer.py:430-433: a `module.` key the network itself has stays as it is
    assert R.strip_module_prefix({"module.a": 1, "module.b": 2}, expected={"module.a", "b"}) == {"module.a": 1, "b": 2}


def test_numpy_scalar_checkpoint_needs_the_helper():
    R = _R()
    for path in (SEG_CK, FLOW_CK):
        with pytest.raises(pickle.UnpicklingError):
            torch.load(path, map_location="cpu", weights_only=True)                  # np.float64 losses: refused by plain weights_only
        ck = R.load_reference_checkpoint(path)
        assert ck["epoch"] == 1000
        assert isinstance(ck["plot_stuff"][0][0], np.float64) and isinstance(ck["best_stuff"][1], np.float64)
        assert not set(ck) & {"optimizer_state_dict", "lr_scheduler_state_dict", "amp_grad_scaler"}
        assert all(isinstance(v, torch.Tensor) for v in ck["state_dict"].values())


def test_foreign_globals_are_refused(tmp_path):
    R = _R()
    marker = tmp_path / "ran"

    class Evil:
        def __reduce__(self):
            return (os.system, ("touch %s" % marker,))

    pkl = tmp_path / "plans.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"num_classes": 3, "x": Evil()}, f)
    with pytest.raises(pickle.UnpicklingError):
        R.load_reference_pickle(str(pkl))
    model = tmp_path / "bad.model"
    torch.save({"epoch": 1, "state_dict": {"w": torch.zeros(2)}, "plot_stuff": Evil()}, str(model))
    with pytest.raises(pickle.UnpicklingError):
        R.load_reference_checkpoint(str(model))
    assert not marker.exists()
    # plain data a protocol-3 nnU-Net pickle (the default of Python <= 3.7) names as a global -- set -- still loads
    ok = tmp_path / "ok.pkl"
    with open(ok, "wb") as f:
        pickle.dump({"all_classes": {1, 2, 3}, "spacing": np.array([8.0, 1.5]), "n": np.int64(3)}, f, protocol=3)
    got = R.load_reference_pickle(str(ok))
    assert got["all_classes"] == {1, 2, 3} and got["n"] == 3 and np.array_equal(got["spacing"], [8.0, 1.5])


def test_values_the_build_cannot_honour_raise_naming_the_key():
    R = _R()
    plans = R.load_reference_pickle(os.path.join(SEG, "plans.pkl"))
    three_d = dict(plans, plans_per_stage={0: dict(plans["plans_per_stage"][0], patch_size=np.array([16, 64, 64]))})
    with pytest.raises(NotImplementedError, match="patch_size"):
        R.plans_from_reference(three_d)
    k5 = dict(plans, plans_per_stage={0: dict(plans["plans_per_stage"][0], conv_kernel_sizes=[[5, 5]] * 4)})
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        R.plans_from_reference(k5)
    with pytest.raises(NotImplementedError, match="conv_per_stage"):
        R.plans_from_reference(dict(plans, conv_per_stage=3))
    two = dict(plans, plans_per_stage={0: plans["plans_per_stage"][0], 1: plans["plans_per_stage"][0]})
    with pytest.raises(ValueError, match="stage"):
        R.plans_from_reference(two)
    assert R.plans_from_reference(two, stage=1)["stage"] == 1


def test_import_writes_the_plans_json_format(tmp_path):
    R = _R()
    from cineflow.predict import CineTrainer
    seg, flow = _copy_tree(tmp_path)
    with open(os.path.join(seg, "postprocessing.json"), "w") as f:
        json.dump({"for_which_classes": [1, 2, 3]}, f)
    out = str(tmp_path / "out")
    R.main(["-s", seg, "-w", os.path.join(flow, "Task031_x"), "-o", out, "--crop_size", "64", "--image_size", "64"])
    with open(os.path.join(out, "plans.json")) as f:
        plans = json.load(f)
    assert plans["flow_net"] == {"config": "config.yaml"} and "cropping_net" not in plans
    assert plans["crop_size"] == 64 and plans["patch_size"] == [64, 64] and plans["num_classes"] == 4
    assert sorted(os.listdir(out)) == ["config.yaml", "fold_0", "plans.json", "postprocessing.json"]
    ck = torch.load(os.path.join(out, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    ref_seg = R.load_reference_checkpoint(SEG_CK)["state_dict"]
    ref_flow = R.load_reference_checkpoint(FLOW_CK)["state_dict"]
    assert set(ck["seg_state_dict"]) == set(ref_seg)
    assert all(torch.equal(ck["seg_state_dict"][k], ref_seg[k]) for k in ref_seg)
    assert set(ck["flow_state_dict"]) == {k for k in ref_flow if not k.endswith("grid")}
    assert all(torch.equal(v, ref_flow[k]) for k, v in ck["flow_state_dict"].items())
    tr = CineTrainer(plans, torch.device("cpu"), model_folder=out)                  # the folder's plans build the networks checked against
    assert set(tr.flow_net.state_shapes()) - {k for k in ref_flow} == set()
    # the task-number rule applies without overrides (Task031 -> crop 128, image 224)
    out2 = str(tmp_path / "out2")
    p2 = R.import_reference_model_folder(seg, flow, out2)
    assert (p2["crop_size"], p2["image_size"], p2["patch_size"]) == (128, 224, [224, 224])


def test_dropped_surplus_and_misshaped_tensors_are_named(tmp_path):
    R = _R()
    seg, flow = _copy_tree(tmp_path)
    seg_ck = os.path.join(seg, "fold_0", "model_final_checkpoint.model")
    flow_ck = os.path.join(flow, "Task031_x", "fold_0", "model_final_checkpoint.model")
    name = "module.seg_outputs.2.weight"
    _rewrite_checkpoint(seg_ck, lambda sd: sd.pop(name))
    out = str(tmp_path / "out")
    with pytest.raises(KeyError, match="seg_outputs.2.weight"):
        R.import_reference_model_folder(seg, flow, out, crop_size=64, image_size=64)
    assert not os.path.exists(out)                                                   # nothing written before every tensor is checked
    shutil.copy(SEG_CK, seg_ck)

    def grow(sd):
        sd["flow_decoder.extra.weight"] = torch.zeros(3)
    _rewrite_checkpoint(flow_ck, grow)
    with pytest.raises(ValueError, match="flow_decoder.extra.weight"):
        R.import_reference_model_folder(seg, flow, out, crop_size=64, image_size=64)
    shutil.copy(FLOW_CK, flow_ck)
    key = sorted(k for k in R.load_reference_checkpoint(FLOW_CK)["state_dict"] if k.endswith("weight"))[0]

    def reshape(sd):
        sd[key] = torch.zeros(tuple(sd[key].shape) + (1,))
    _rewrite_checkpoint(flow_ck, reshape)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        R.import_reference_model_folder(seg, flow, out, crop_size=64, image_size=64)
    assert not os.path.exists(out)


def test_folds_must_be_present_on_both_sides(tmp_path):
    R = _R()
    seg, flow = _copy_tree(tmp_path)
    shutil.copytree(os.path.join(seg, "fold_0"), os.path.join(seg, "fold_1"))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="different folds"):
        R.import_reference_model_folder(seg, flow, out, crop_size=64, image_size=64)
    with pytest.raises(FileNotFoundError, match="fold_1"):
        R.import_reference_model_folder(seg, flow, out, folds=[1], crop_size=64, image_size=64)
    assert not os.path.exists(out)
    R.import_reference_model_folder(seg, flow, out, folds=[0], crop_size=64, image_size=64)
    assert os.listdir(os.path.join(out)) and os.path.isdir(os.path.join(out, "fold_0")) and not os.path.exists(os.path.join(out, "fold_1"))
    with pytest.raises(FileNotFoundError):
        R.import_reference_model_folder(seg, os.path.join(flow, "missing"), str(tmp_path / "o3"))


def test_import_with_the_mtl_cropper(tmp_path):
    """crop_weights / crop_config: the MTLmodel cropper's reference checkpoint ({'state_dict': ...} with its BatchNorm counters and Swin
    index / mask buffers) and its YAML go into plans['cropping_net'] and the folds' crop_state_dict"""
    import yaml
    R = _R()
    from cineflow.predict import CineTrainer
    from cineflow.weights import seeded_state_dict
    seg, flow = _copy_tree(tmp_path)
    with open(os.path.join(HERE, "golden", "configs.json")) as f:
        cfg = dict(json.load(f)["adversarial_acdc"]["values"], in_encoder_dims=[1, 16, 32], out_encoder_dims=[8, 16, 32],
                   spatial_cross_attention_num_heads=[2, 2, 4])
    crop_yaml = str(tmp_path / "adversarial_acdc.yaml")
    with open(crop_yaml, "w") as f:
        yaml.safe_dump(cfg, f)
    probe = CineTrainer({"num_modalities": 1, "num_classes": 4, "patch_size": [96, 96], "mirror_axes": [0, 1], "crop_size": 64,
                         "seg_net": {"base_num_features": 8, "num_pool": 3}, "flow_net": {"variant": "video", "kwargs": {}},
                         "cropping_net": {"type": "mtl", "config": cfg, "window_size": 8}}, torch.device("cpu"))
    shapes = probe.crop_net.state_shapes()
    sd = {"module." + k: v for k, v in seeded_state_dict(shapes, 53).items()}
    sd["module.decoder.x.num_batches_tracked"] = torch.tensor(5)                       # a derived buffer: ignored
    crop_ck = str(tmp_path / "model_final_checkpoint.model")
    torch.save({"epoch": 10, "state_dict": sd, "optimizer_state_dict": None, "plot_stuff": ([np.float64(0.5)],)}, crop_ck)
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="go together"):
        R.import_reference_model_folder(seg, flow, out, crop_weights=crop_ck, crop_size=64, image_size=96, window_size=8)
    plans = R.import_reference_model_folder(seg, flow, out, crop_weights=crop_ck, crop_config=crop_yaml, crop_size=64, image_size=96,
                                            window_size=8)
    assert plans["cropping_net"] == {"type": "mtl", "config": "cropping_config.yaml", "window_size": 8}
    assert os.path.isfile(os.path.join(out, "cropping_config.yaml"))
    ck = torch.load(os.path.join(out, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    assert set(ck["crop_state_dict"]) == {k[len("module."):] for k in sd} - {"decoder.x.num_batches_tracked"}
