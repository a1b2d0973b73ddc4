"""CPU tests (no GPU) of nnMTLTrainerV2 model folders: plans with seg_net.arch = 'mtl' in CineTrainer, what it refuses, the importer on
tests/golden/ref_model_folder_mtl (written by the reference's own save_checkpoint, make_golden_mtl_folder.py), the host-side argument
checks of cf_crop_windows / cf_tta_accumulate_window, and cf_crop_windows' integer arithmetic restated in numpy against the Processor."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import _mtl_folder_fixture as FX
from _crop_window_cases import SIZES, cases, windows_numpy

CPU = torch.device("cpu")


def test_cine_trainer_builds_an_mtl_segmenter_behind_its_cropper():
    """(on the parent commit: ValueError "seg_net.arch must be 'resenc' ...")"""
    from cineflow.inference import Processor
    from cineflow.mtl import MTLmodel
    from cineflow.trainer import CineTrainer
    seg_cfg, crop_cfg = FX.configs()
    t = CineTrainer(FX.mtl_plans(seg_cfg, crop_cfg, normalize=True), CPU)
    assert isinstance(t.seg_net, MTLmodel) and t.seg_net.num_classes == 4 and t.seg_net.image_size == 64 and t.seg_net.normalize is True
    assert isinstance(t.crop_net, MTLmodel) and t.crop_net.num_classes == 2 and t.crop_net.image_size == 96
    assert isinstance(t.processor, Processor) and t.seg_net._processor is t.processor and t.processor.cropping_network is t.crop_net
    assert (t.processor.crop_size, t.processor.image_size) == (64, 96)
    assert t.flow_net is None and t.seg_dim == 2 and t.seg_arch == "mtl" and t.patch_size == (96, 96)
    other = t._new_seg_net()                                                      # a further fold: its own weights, the same Processor
    assert other is not t.seg_net and other._processor is t.processor
    # without a cropping network the segmenter runs on the whole image (nnMTLTrainerV2.py:608-610) and has no Processor
    t = CineTrainer(FX.mtl_plans(seg_cfg, None), CPU)
    assert t.seg_net.image_size == 96 and t.processor is None and t.crop_net is None and t.seg_net._processor is None and t.seg_net.normalize is False


def test_cine_trainer_refuses_what_an_mtl_folder_cannot_hold():
    from cineflow.trainer import CineTrainer, default_plans
    seg_cfg, crop_cfg = FX.configs()
    good = FX.mtl_plans(seg_cfg, crop_cfg)

    def refused(change, *words):
        p = copy.deepcopy(good)
        change(p)
        with pytest.raises(ValueError) as e:
            CineTrainer(p, CPU)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    refused(lambda p: p["seg_net"].update(dim=3, ), "seg_net.arch", "seg_net.dim")
    refused(lambda p: p.update(flow_net=default_plans(64, 64)["flow_net"]), "seg_net.arch", "flow_net")
    refused(lambda p: p["seg_net"].update(prev_stage_classes=[1, 2, 3]), "seg_net.arch", "prev_stage_classes")
    refused(lambda p: p.update(patch_size=[96, 64]), "patch_size", "image_size")
    refused(lambda p: p.update(patch_size=[64, 64]), "patch_size", "image_size")
    refused(lambda p: p.pop("crop_size"), "cropping_net", "crop_size")
    refused(lambda p: p["seg_net"].update(arch="swin"), "seg_net.arch")
    # what build_2d_model refuses keeps its NotImplementedError
    for key, value in (("transformer_depth", [2]), ("norm", "GroupNorm"), ("reconstruction", True)):
        p = copy.deepcopy(good)
        p["seg_net"]["config"][key] = value
        with pytest.raises(NotImplementedError):
            CineTrainer(p, CPU)


def _import(src, out, **kw):
    from cineflow import reference_models as RM
    args = dict(seg_config=os.path.join(src, "seg_config.yaml"), crop_weights=os.path.join(src, "binary", "model_final_checkpoint.model"),
                crop_config=os.path.join(src, "cropping_config.yaml"), crop_size=64, window_size=8)
    args.update(kw)
    return RM.import_reference_model_folder(os.path.join(src, "seg"), None, out, **args)


def test_importer_on_the_reference_written_folder_equals_a_save_model_folder_twin(tmp_path):
    from cineflow import reference_models as RM
    from cineflow.trainer import CineTrainer, load_model_and_checkpoint_files, save_model_folder
    from cineflow.weights import seeded_state_dict
    src = FX.unpack(str(tmp_path / "src"))
    info = RM.load_reference_pickle(os.path.join(src, "seg", "fold_0", "model_final_checkpoint.model.pkl"))
    assert info["name"] == "nnMTLTrainerV2"
    out = str(tmp_path / "out")
    plans = _import(src, out)
    assert sorted(os.listdir(out)) == ["cropping_config.yaml", "fold_0", "fold_1", "plans.json", "seg_config.yaml"]
    assert plans["seg_net"] == {"arch": "mtl", "config": "seg_config.yaml", "window_size": 8, "normalize": False}
    assert plans["cropping_net"] == {"type": "mtl", "config": "cropping_config.yaml", "window_size": 8}
    assert (plans["image_size"], plans["crop_size"], plans["patch_size"], plans["num_classes"]) == (96, 64, [96, 96], 4)
    # the twin: the same plans by hand, seeded weights through save_model_folder
    twin = str(tmp_path / "twin")
    tp = FX.mtl_plans("seg_config.yaml", "cropping_config.yaml")
    os.makedirs(twin)
    for n in ("seg_config.yaml", "cropping_config.yaml"):
        with open(os.path.join(FX.TREE, n), "rb") as f, open(os.path.join(twin, n), "wb") as g:
            g.write(f.read())
    t = CineTrainer(tp, CPU, model_folder=twin)
    for fold in (0, 1):
        save_model_folder(twin, t.seg_net, None, tp, fold=fold, seg_sd=seeded_state_dict(t.seg_net.state_shapes(), 5 + fold),
                          crop_sd=seeded_state_dict(t.crop_net.state_shapes(), 9))
    with open(os.path.join(out, "plans.json")) as f, open(os.path.join(twin, "plans.json")) as g:
        got, want = json.load(f), json.load(g)
    for k, v in want.items():                                                    # (the import also keeps the planner's preprocessing entries)
        assert got[k] == v, k
    assert set(got) - set(want) <= {"normalization_schemes", "use_mask_for_norm", "dataset_properties", "preprocessor_name", "plans_per_stage", "stage"}
    _tr, a = load_model_and_checkpoint_files(out, None, device=CPU)
    _tw, b = load_model_and_checkpoint_files(twin, None, device=CPU)
    assert len(a) == len(b) == 2
    for pa, pb in zip(a, b):
        assert sorted(pa) == sorted(pb) == ["crop_state_dict", "seg_state_dict"]
        for part in pa:
            assert {k: tuple(v.shape) for k, v in pa[part].items()} == {k: tuple(v.shape) for k, v in pb[part].items()}
    assert not torch.equal(a[0]["seg_state_dict"]["encoder.layers.0.blocks.0.0.weight"], a[1]["seg_state_dict"]["encoder.layers.0.blocks.0.0.weight"])
    assert all(torch.equal(a[0]["crop_state_dict"][k], a[1]["crop_state_dict"][k]) for k in a[0]["crop_state_dict"])
    # the weights are the reference file's
    ref = RM.load_reference_checkpoint(os.path.join(src, "seg", "fold_1", "model_final_checkpoint.model"))["state_dict"]
    assert all(torch.equal(v, ref[k]) for k, v in a[1]["seg_state_dict"].items())
    # fold selection
    one = str(tmp_path / "one")
    _import(src, one, folds=[1])
    assert sorted(d for d in os.listdir(one) if d.startswith("fold_")) == ["fold_1"]


def test_importer_refusals_leave_no_output_folder(tmp_path):
    from cineflow import reference_models as RM
    src = FX.unpack(str(tmp_path / "src"))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="config.yaml"):                         # no --seg_config: names the trainer's config.yaml
        _import(src, out, seg_config=None)
    with pytest.raises(ValueError, match="crop_weights and crop_config"):        # cropper: true without the cropper
        _import(src, out, crop_weights=None, crop_config=None)
    with pytest.raises(ValueError, match="crop_weights and crop_config"):
        _import(src, out, crop_config=None)
    with pytest.raises(ValueError, match="window_size"):                         # nnMTLTrainerV2.py:121 has no window for image 96
        _import(src, out, window_size=None)
    with pytest.raises(ValueError, match="flow folder"):
        RM.import_reference_model_folder(os.path.join(src, "seg"), os.path.join(src, "binary"), out, seg_config=os.path.join(src, "seg_config.yaml"))
    # a renamed tensor and a wrong shape in the SECOND fold, and in the cropper: nothing is written before every fold has passed
    path = os.path.join(src, "seg", "fold_1", "model_final_checkpoint.model")
    with torch.serialization.safe_globals(RM._numpy_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    good = dict(ck["state_dict"])
    name = "decoder.layers.2.blocks.0.0.weight"
    ck["state_dict"] = {("renamed." + k if k == name else k): v for k, v in good.items()}
    torch.save(ck, path)
    with pytest.raises(KeyError, match=name):
        _import(src, out)
    ck["state_dict"] = dict(good, **{name: good[name][:, :-1].contiguous()})
    torch.save(ck, path)
    with pytest.raises(ValueError, match="another shape"):
        _import(src, out)
    ck["state_dict"] = dict(good, surplus=torch.zeros(3))
    torch.save(ck, path)
    with pytest.raises(ValueError, match="does not have"):
        _import(src, out)
    with pytest.raises(ValueError, match="another shape"):                       # a 4-class network is no cropper
        _import(src, out, folds=[0], crop_weights=os.path.join(src, "seg", "fold_0", "model_final_checkpoint.model"))
    assert not os.path.exists(out)
    _import(src, out, folds=[0])                                                  # the untouched fold still imports
    assert os.path.isfile(os.path.join(out, "fold_0", "model_final_checkpoint.model"))


def test_size_rules_of_the_trainer():
    from cineflow import reference_models as RM
    assert [RM.mtl_window_size(s) for s in (224, 288, 384, 192, 96)] == [7, 9, 8, 8, None]          # nnMTLTrainerV2.py:121
    assert [RM.mtl_crop_size(t) for t in ("Task031_ACDC", "Task035_x", "Task032_Lib", "Task045_q")] == [128, 128, 192, 192]   # :110-117


@pytest.mark.parametrize("image,crop", SIZES)
def test_window_arithmetic_in_numpy_equals_the_processor(image, crop):
    """cf_crop_windows' documented integers (tests/_crop_window_cases.windows_numpy) against Processor.get_mean_centroid for one frame +
    adjust_cropping_window on every case of tests/test_gpu_crop_windows.py"""
    from oracle import models as OM
    proc = OM.Processor(crop, image)
    for name, m in cases(image):
        want = proc.adjust_cropping_window(proc.get_mean_centroid(torch.from_numpy(m[None]).long()))["crop_indices"]
        win, jobs = windows_numpy(m[None], crop, image)
        assert win[0].tolist() == list(want), (name, win[0], want)
        assert jobs[0].tolist() == [0, want[2], want[0]] and want[1] - want[0] == crop and want[3] - want[2] == crop, name
        assert 0 <= want[0] <= image - crop and 0 <= want[2] <= image - crop, name
    # both clamps, the .5 truncation and the empty map's centre are really among the cases
    wins = {n: windows_numpy(m[None], crop, image)[0][0].tolist() for n, m in cases(image)}
    assert wins["corner_tl"] == [0, crop, 0, crop] and wins["corner_br"] == [image - crop, image, image - crop, image]
    assert wins["empty"][0] == max(0, min(image - crop, image // 2 - crop // 2))


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """every argument error is caught on the host (-1 and a message); the non-null pointers are never dereferenced"""
    from cineflow import _lib, ops
    h = _lib.lib()
    p = 4096
    assert h.cf_crop_windows(None, p, p, 1, 12, 12, 8, 12, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_crop_windows(p, p, None, 1, 12, 12, 8, 12, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_crop_windows(p, p, p, 0, 12, 12, 8, 12, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_crop_windows(p, p, p, 1, 12, 12, 7, 12, None) == -1 and b"even" in h.cf_last_error()           # Processor.crop_and_pad cuts 2 * (crop // 2)
    assert h.cf_crop_windows(p, p, p, 1, 12, 12, 14, 12, None) == -1 and b"bad window" in h.cf_last_error()    # crop > image
    assert h.cf_crop_windows(p, p, p, 1, 12, 10, 8, 12, None) == -1 and b"bad window" in h.cf_last_error()     # image > W: a window could leave the map
    assert h.cf_tta_accumulate_window(None, p, p, 1, 2, 8, 12, 12, 0, 0, 0.25, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tta_accumulate_window(p, None, p, 1, 2, 8, 12, 12, 0, 0, 0.25, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tta_accumulate_window(p, p, p, 1, 0, 8, 12, 12, 0, 0, 0.25, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_tta_accumulate_window(p, p, p, 1, 2, 13, 12, 12, 0, 0, 0.25, None) == -1 and b"bad shape" in h.cf_last_error()
    with pytest.raises(TypeError):
        ops.crop_windows(torch.zeros(1, 12, 12, dtype=torch.uint8), 8, 12)
    with pytest.raises(TypeError):
        ops.tta_accumulate_window(torch.zeros(1, 2, 8, 8), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 2, 12, 12), 0, 0, 0.25)
