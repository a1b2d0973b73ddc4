"""A two-fold seg_net.arch = 'mtl' model folder through predict_from_folder: two synthetic patients of 2 frames x 3 slices, one of
96 x 96 slices (one tile) and one of 130 x 96 slices (two tiles, Gaussian weighting), against the oracle's tiled prediction with the
oracle's per-sample wrapper as the tile network and the fold mean (tests/_mtl_oracle.py); then the reference-written fixture folder,
imported, against its save_model_folder twin, byte for byte.

Bars.  Softmax within 5e-5 of the oracle (the project's MTLmodel bound, tests/test_mtl.py).  The `-z` file holds the softmax as float16
(predict.py's export), so the file is held to 5e-5 plus half a float16 step of the stored value, and the float32 softmax of the same
trainer call (predict_preprocessed_data_return_seg_and_softmax) to 5e-5 itself.  Labels are equal wherever the oracle's top-two softmax
gap is at least 1e-3, and ALSO wherever the oracle's softmax is zero in every class -- outside every crop window, 55 % of a one-tile
slice, where the gap is 0 by construction (uncrop_no_registration's F.pad) and the label is 0: counting that region as excluded would
break the 0.5 % cap for any implementation, so it is compared instead.  At most 0.5 % of the voxels may be excluded (a cap).

Seeds (chosen on the CPU, tests/_mtl_oracle.py's generators): cropper 73, folds 11 and 12, patients 2096 and 2131.  On the preprocessed
frames the oracle's float32 and float64 cropper label maps are equal on every one of the 18 tiles, the smallest top-two logit gap of the
cropper is 1.676e-02 (>= 1e-3: no window can flip), 0.3441 % of the 130 176 voxels have a top-two softmax gap below 1e-3 inside a
window and are excluded, and the oracle's float32 and float64 labels disagree at no voxel at all."""
import os

import numpy as np
import pytest
import torch

import _mtl_folder_fixture as FX
import _mtl_oracle as MO

pytestmark = pytest.mark.gpu

CROP_SEED, SEG_SEEDS = 73, (11, 12)
PATIENTS = {"patient001": (96, 96, 2096), "patient002": (130, 96, 2131)}
T, Z = 2, 3
BOUND, GAP, CAP = 5e-5, 1e-3, 0.005


def _write_patients(inp):
    from cineflow.nifti import write_nifti
    for pat, (Y, X, seed) in PATIENTS.items():
        os.makedirs(os.path.join(inp, pat))
        vols = MO.patient_volumes(Y, X, seed, T, Z)
        for t in range(T):
            write_nifti(os.path.join(inp, pat, "%s_frame%02d_0000.nii.gz" % (pat, t)), vols[t], (1.5, 1.5, 8.0), (0, 0, 0))


def _seeded_folder(folder):
    from cineflow.trainer import CineTrainer, save_model_folder
    from cineflow.weights import seeded_state_dict
    seg_cfg, crop_cfg = FX.configs()
    plans = FX.mtl_plans(seg_cfg, crop_cfg)
    t = CineTrainer(plans, torch.device("cpu"))
    for fold, s in enumerate(SEG_SEEDS):
        save_model_folder(folder, t.seg_net, None, plans, fold=fold, seg_sd=seeded_state_dict(t.seg_net.state_shapes(), s),
                          crop_sd=seeded_state_dict(t.crop_net.state_shapes(), CROP_SEED))


def _tree(folder):
    out = {}
    for root, _dirs, files in os.walk(folder):
        for fn in files:
            with open(os.path.join(root, fn), "rb") as f:
                out[os.path.relpath(os.path.join(root, fn), folder)] = f.read()
    return out


def test_two_fold_mtl_folder_vs_the_oracles_tiled_prediction(dev, tmp_path):
    from cineflow import predict as P
    from cineflow.nifti import read_nifti
    model, inp, out = str(tmp_path / "model"), str(tmp_path / "in"), str(tmp_path / "out")
    _seeded_folder(model)
    _write_patients(inp)
    res = P.predict_from_folder(model, inp, out, None, True, 1, 1, None, 0, 1, True)
    assert sorted(res) == sorted(PATIENTS)
    ocrop, osegs = MO.oracle_nets(CROP_SEED, SEG_SEEDS)
    trainer, params = P.load_model_and_checkpoint_files(model, None, device=dev)
    trainer.load_ensemble(params)
    assert len(trainer.seg_nets) == 2 and trainer.seg_nets[0]._processor is trainer.seg_nets[1]._processor
    excluded = total = 0
    worst_file, worst_f32 = -1.0, 0.0
    for pat, (Y, X, _seed) in PATIENTS.items():
        assert sorted(os.listdir(os.path.join(out, pat))) == sorted("%s_frame%02d%s" % (pat, t, e) for t in range(T) for e in (".nii.gz", ".npz", ".pkl"))
        for t in range(T):
            case = "%s_frame%02d" % (pat, t)
            d, _sg, _props = trainer.preprocess_patient([os.path.join(inp, pat, case + "_0000.nii.gz")])
            assert d.shape == (1, Z, Y, X)
            want = MO.oracle_tiled(ocrop, osegs, np.asarray(d, dtype=np.float32))                     # [4,Z,Y,X]
            seg32, soft32 = trainer.predict_preprocessed_data_return_seg_and_softmax(d)
            worst_f32 = max(worst_f32, float(np.abs(soft32 - want).max()))
            sm = np.load(os.path.join(out, pat, case + ".npz"))["softmax"]
            assert sm.shape == want.shape and sm.dtype == np.float16
            slack = BOUND + np.spacing(np.abs(sm)).astype(np.float64) / 2
            over = np.abs(sm.astype(np.float64) - want) - slack
            worst_file = max(worst_file, float(over.max()))
            lab, _ = read_nifti(os.path.join(out, pat, case + ".nii.gz"))
            assert lab.shape == (Z, Y, X) and lab.dtype == np.uint8
            top = np.sort(want, 0)[::-1]
            zero = top[0] == 0                                                    # outside every window: zeros in every class
            sure = ((top[0] - top[1]) >= GAP) | zero
            assert np.array_equal(lab[sure], want.argmax(0)[sure].astype(np.uint8)), case
            assert np.array_equal(seg32[sure], want.argmax(0)[sure]), case
            assert not lab[zero].any() and not soft32[:, zero].any(), case
            excluded += int((~sure).sum())
            total += sure.size
    print("float32 softmax vs oracle %.3e; -z file beyond 5e-5 + half a float16 step: %.3e; excluded %.4f %% of %d voxels"
          % (worst_f32, worst_file, 100.0 * excluded / total, total))
    assert worst_f32 <= BOUND, worst_f32
    assert worst_file <= 0.0, worst_file
    assert excluded <= CAP * total, (excluded, total)
    # two runs write the same bytes
    out2 = str(tmp_path / "out2")
    P.predict_from_folder(model, inp, out2, None, True, 1, 1, None, 0, 1, True)
    a, b = _tree(out), _tree(out2)
    assert sorted(a) == sorted(b)
    assert [k for k in a if a[k] != b[k]] == []


def test_imported_fixture_folder_writes_the_bytes_of_its_save_model_folder_twin(dev, tmp_path):
    from cineflow import predict as P
    from cineflow import reference_models as RM
    from cineflow.trainer import save_model_folder
    src = FX.unpack(str(tmp_path / "src"))
    model = str(tmp_path / "imported")
    plans = RM.import_reference_model_folder(os.path.join(src, "seg"), None, model, seg_config=os.path.join(src, "seg_config.yaml"),
                                             crop_weights=os.path.join(src, "binary", "model_final_checkpoint.model"),
                                             crop_config=os.path.join(src, "cropping_config.yaml"), crop_size=64, window_size=8)
    assert plans["seg_net"]["arch"] == "mtl"
    # the twin: hand-written plans with the YAML values inline, the reference files' tensors through save_model_folder
    twin = str(tmp_path / "twin")
    seg_cfg, crop_cfg = FX.configs()
    tp = FX.mtl_plans(seg_cfg, crop_cfg)
    drop = ("num_batches_tracked", "relative_position_index", "attn_mask")
    crop_sd = RM.load_reference_checkpoint(os.path.join(src, "binary", "model_final_checkpoint.model"))["state_dict"]
    for fold in (0, 1):
        sd = RM.load_reference_checkpoint(os.path.join(src, "seg", "fold_%d" % fold, "model_final_checkpoint.model"))["state_dict"]
        save_model_folder(twin, None, None, tp, fold=fold, seg_sd={k: v for k, v in sd.items() if not k.endswith(drop)},
                          crop_sd={k: v for k, v in crop_sd.items() if not k.endswith(drop)})
    inp = str(tmp_path / "in")
    _write_patients(inp)
    outs = {}
    for tag, m in (("imported", model), ("twin", twin)):
        outs[tag] = str(tmp_path / ("out_" + tag))
        P.predict_from_folder(m, inp, outs[tag], None, True, 1, 1, None, 0, 1, True)
    a, b = _tree(outs["imported"]), _tree(outs["twin"])
    # (predict_from_folder also copies the model's plans.json into the output folder: the two folders' plans say the same in other words
    # -- file names against inline values, the planner's preprocessing entries -- so that copy is the one file left out)
    assert a.pop("plans.json") != b.pop("plans.json")
    assert sorted(a) == sorted(b) and len(a) == 3 * T * len(PATIENTS)
    assert [k for k in a if a[k] != b[k]] == []
    # fold selection and -z off: label files of the chosen fold alone
    one = str(tmp_path / "out_fold1")
    res = P.predict_from_folder(model, inp, one, [1], False, 1, 1, None, 1, 2, True)
    assert sorted(res) == ["patient002"] and sorted(os.listdir(os.path.join(one, "patient002"))) == ["patient002_frame%02d.nii.gz" % t for t in range(T)]
    assert any(a["patient002/patient002_frame%02d.nii.gz" % t] != _tree(one)["patient002/patient002_frame%02d.nii.gz" % t] for t in range(T))
