"""A `3d_cascade_fullres` folder written by the reference's trainer, host side: the importer's cascade detection, the plans entry
seg_net.prev_stage_classes and its refusals, the lowres folder of the same two-stage plans, the lookup of the previous stage's label
files in predict_from_folder (before any model load), and the ABI of the new entry point.

The fixture tree tests/golden/ref_model_folder_cascade/ was written by the reference's own save_checkpoint
(make_golden_refckpt_cascade.py): fold_0 holds a Generic_UNet(1 + 3, ..., nn.Conv3d) saved as nnUNetTrainerV2CascadeFullRes with
init[5] = 1, lowres/ the one-channel stage-0 network with init[5] = 0."""
import json
import os
import shutil

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASCADE = os.path.join(HERE, "golden", "ref_model_folder_cascade")
LOWRES = os.path.join(CASCADE, "lowres")
FIRST = "conv_blocks_context.0.blocks.0.conv.weight"


def _R():
    from cineflow import reference_models
    return reference_models


def _rewrite(path, edit_sd=None, edit_info=None):
    R = _R()
    if edit_sd is not None:
        with torch.serialization.safe_globals(R._numpy_safe_globals()):
            ck = torch.load(path, map_location="cpu", weights_only=True)
        edit_sd(ck["state_dict"])
        torch.save(ck, path)
    if edit_info is not None:
        import pickle
        info = R.load_reference_pickle(path + ".pkl")
        edit_info(info)
        with open(path + ".pkl", "wb") as f:
            pickle.dump(info, f)


def _cascade_plans():
    R = _R()
    p = R.plans_from_reference_3d(R.load_reference_pickle(os.path.join(CASCADE, "plans.pkl")), 1)
    p["seg_net"]["prev_stage_classes"] = [1, 2, 3]
    return p


def test_the_cascade_fixture_imports_with_prev_stage_classes(tmp_path):
    from cineflow.models import Generic_UNet3D
    from cineflow.predict import CineTrainer
    out = str(tmp_path / "out")
    _R().main(["-s", CASCADE, "-o", out])
    with open(os.path.join(out, "plans.json")) as f:
        plans = json.load(f)
    assert plans["seg_net"]["prev_stage_classes"] == [1, 2, 3] and plans["seg_net"]["dim"] == 3 and plans["stage"] == 1
    assert plans["num_modalities"] == 1 and plans["num_classes"] == 4 and "flow_net" not in plans
    assert plans["plans_per_stage"]["1"]["current_spacing"] == [10.0, 1.5, 1.5]
    trainer = CineTrainer(plans, torch.device("cpu"), model_folder=out)
    assert isinstance(trainer.seg_net, Generic_UNet3D) and trainer.seg_net.input_channels == 4 and trainer.prev_stage_classes == [1, 2, 3]
    ck = torch.load(os.path.join(out, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    assert {k: tuple(v.shape) for k, v in ck["seg_state_dict"].items()} == trainer.seg_net.state_shapes()
    assert tuple(ck["seg_state_dict"][FIRST].shape) == (4, 4, 1, 3, 3)


def test_the_lowres_folder_of_the_same_plans_imports_as_stage_0(tmp_path):
    out = str(tmp_path / "low")
    plans = _R().import_reference_model_folder(LOWRES, None, out)
    assert plans["stage"] == 0 and "prev_stage_classes" not in plans["seg_net"] and plans["seg_net"]["dim"] == 3
    assert plans["plans_per_stage"]["0"]["current_spacing"] == [10.0, 2.0, 2.0] and plans["patch_size"] == [8, 32, 32]
    ck = torch.load(os.path.join(out, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    assert tuple(ck["seg_state_dict"][FIRST].shape) == (4, 1, 1, 3, 3)


def test_the_first_convolution_width_alone_marks_a_cascade(tmp_path):
    """no `Cascade` in the trainer's name (a custom trainer class): num_modalities + num_classes input channels decide"""
    seg = str(tmp_path / "seg")
    shutil.copytree(CASCADE, seg)

    def rename(info):
        info["name"] = "MyTrainer"
    _rewrite(os.path.join(seg, "fold_0", "model_final_checkpoint.model"), edit_info=rename)
    plans = _R().import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert plans["seg_net"]["prev_stage_classes"] == [1, 2, 3]


@pytest.mark.parametrize("width, name", [(3, "MyTrainer"), (2, "MyTrainer"), (5, "MyTrainer"), (3, "nnUNetTrainerV2CascadeFullRes")])
def test_any_other_first_convolution_width_still_raises(tmp_path, width, name):
    seg = str(tmp_path / "seg")
    shutil.copytree(CASCADE, seg)
    key = "module." + FIRST

    def edit(sd):
        w = sd.get(key, sd.get(FIRST))
        new = torch.cat([w, w], 1)[:, :width].contiguous()
        sd[key if key in sd else FIRST] = new

    def rename(info):
        info["name"] = name
    _rewrite(os.path.join(seg, "fold_0", "model_final_checkpoint.model"), edit, rename)
    with pytest.raises(ValueError, match="conv_blocks_context.0.blocks.0.conv.weight"):
        _R().import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_prev_stage_classes_is_refused_for_2d_models_and_next_to_a_flow_net():
    from cineflow.predict import CineTrainer, default_plans
    p2 = default_plans(image_size=32, crop_size=16, seg_base=4, seg_pool=2)
    p2.pop("flow_net", None)
    p2["seg_net"]["prev_stage_classes"] = [1, 2, 3]
    with pytest.raises(ValueError, match="prev_stage_classes"):
        CineTrainer(p2, torch.device("cpu"))
    p3 = _cascade_plans()
    p3["flow_net"] = {"variant": "video", "kwargs": {}}
    p3["crop_size"] = 32
    with pytest.raises(ValueError, match="flow_net"):
        CineTrainer(p3, torch.device("cpu"))
    for bad in ([], [1, "2"], [1, 300], "123"):
        p = _cascade_plans()
        p["seg_net"]["prev_stage_classes"] = bad
        with pytest.raises(ValueError, match="prev_stage_classes"):
            CineTrainer(p, torch.device("cpu"))
    t = CineTrainer(_cascade_plans(), torch.device("cpu"))
    assert t.seg_net.state_shapes()[FIRST] == (4, 4, 1, 3, 3)


def test_model_and_previous_stage_mismatches_raise_value_errors(tmp_path):
    from cineflow.predict import CineTrainer
    t = CineTrainer(_cascade_plans(), torch.device("cpu"), model_folder="/models/cascade")
    with pytest.raises(ValueError, match="-l"):
        t.preprocess_patient(["x_0000.nii.gz"])
    plain = _cascade_plans()
    del plain["seg_net"]["prev_stage_classes"]
    t = CineTrainer(plain, torch.device("cpu"), model_folder="/models/fullres")
    with pytest.raises(ValueError, match="/models/fullres"):
        t.preprocess_patient(["x_0000.nii.gz"], "prev.nii.gz")


# ------------------------------------------------------------------------------------------------ predict_from_folder's -l lookup
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb"):
        pass


@pytest.fixture()
def folders(tmp_path):
    """a model folder with plans.json and NO checkpoint (any model load would raise), two patients with two frames each"""
    model = tmp_path / "model"
    model.mkdir()
    with open(str(model / "plans.json"), "w") as f:
        json.dump(_cascade_plans(), f)
    inp = tmp_path / "in"
    for pat in ("patient001", "patient002"):
        for t in range(2):
            _touch(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))))
    return str(model), str(inp), tmp_path


def _predict(model, inp, out, lowres):
    from cineflow import predict as P
    return P.predict_from_folder(model, inp, str(out), [0], False, 1, 1, lowres, 0, 1, True)


def test_lowres_segmentations_must_be_a_directory(folders):
    model, inp, tmp = folders
    f = str(tmp / "seg.nii.gz")
    _touch(f)
    with pytest.raises(AssertionError, match="if lowres_segmentations is not None then it must point to a directory"):
        _predict(model, inp, tmp / "out", f)


@pytest.mark.parametrize("layout", ["per_patient", "flat"])
def test_a_missing_lowres_file_raises_before_the_model_is_loaded(folders, layout):
    model, inp, tmp = folders
    low = tmp / "low"
    cases = [(p, "%s_frame%02d" % (p, t)) for p in ("patient001", "patient002") for t in range(2)]
    for pat, case in cases[:-1]:                                                     # the last case is missing
        _touch(str(low / pat / (case + ".nii.gz")) if layout == "per_patient" else str(low / (case + ".nii.gz")))
    with pytest.raises(AssertionError, match="not all lowres_segmentations files are present"):
        _predict(model, inp, tmp / "out", str(low))
    # with every file present the call gets as far as the model load, which this folder cannot satisfy
    pat, case = cases[-1]
    _touch(str(low / pat / (case + ".nii.gz")) if layout == "per_patient" else str(low / (case + ".nii.gz")))
    with pytest.raises(Exception) as e:
        _predict(model, inp, tmp / "out", str(low))
    assert not isinstance(e.value, AssertionError) or "lowres_segmentations" not in str(e.value)


def test_mismatch_errors_of_predict_from_folder_need_no_model_load(folders):
    model, inp, tmp = folders
    with pytest.raises(ValueError, match="-l"):
        _predict(model, inp, tmp / "out", None)
    plain = _cascade_plans()
    del plain["seg_net"]["prev_stage_classes"]
    with open(os.path.join(model, "plans.json"), "w") as f:
        json.dump(plain, f)
    (tmp / "low").mkdir()
    with pytest.raises(ValueError, match="model"):
        _predict(model, inp, tmp / "out", str(tmp / "low"))


def test_the_per_patient_file_wins_over_the_flat_one(tmp_path):
    from cineflow.predict import lowres_segmentation_file
    low = tmp_path / "low"
    flat, own = str(low / "p1_frame00.nii.gz"), str(low / "p1" / "p1_frame00.nii.gz")
    assert lowres_segmentation_file(str(low), "p1", "p1_frame00") == flat           # neither exists: the reference's literal join
    _touch(flat)
    assert lowres_segmentation_file(str(low), "p1", "p1_frame00") == flat
    _touch(own)
    assert lowres_segmentation_file(str(low), "p1", "p1_frame00") == own


def test_cli_lowres_model_needs_a_single_part(folders):
    from cineflow import predict as P
    model, inp, tmp = folders
    with pytest.raises(AssertionError, match="custom values for part_id and num_parts"):
        P.main(["-i", inp, "-o", str(tmp / "out"), "-m", model, "--lowres_model", model, "--num_parts", "2"])


# ------------------------------------------------------------------------------------------------ ABI
def test_the_new_entry_point_is_declared_bound_and_exported():
    import ctypes
    import re
    from cineflow import _lib, ops
    with open(os.path.join(ROOT, "include", "cineflow.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+cf_prev_stage_onehot\s*\(", header)
    P_, I_ = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["cf_prev_stage_onehot"] == [P_, I_, I_, I_, P_, I_, I_, I_, P_, I_, P_]
    h = _lib.lib()
    assert hasattr(h, "cf_prev_stage_onehot") and callable(ops.prev_stage_onehot)
    # argument errors are caught on the host, before any launch
    cls = (ctypes.c_uint8 * 3)(1, 2, 3)
    cp = ctypes.cast(cls, ctypes.c_void_p)
    assert h.cf_prev_stage_onehot(None, 4, 4, 4, None, 8, 8, 8, cp, 3, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_prev_stage_onehot(16, 4, 4, 0, 16, 8, 8, 8, cp, 3, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_prev_stage_onehot(16, 4, 4, 4, 16, 8, 8, 8, cp, 0, None) == -1 and b"n_classes" in h.cf_last_error()
    assert h.cf_prev_stage_onehot(16, 4, 4, 4, 18, 8, 8, 8, cp, 3, None) == -1 and b"aligned" in h.cf_last_error()
    with pytest.raises(TypeError):
        ops.prev_stage_onehot(torch.zeros(4, 4, 4, dtype=torch.uint8), [1, 2, 3], torch.zeros(3, 8, 8, 8))   # CPU tensors: no CPU path
