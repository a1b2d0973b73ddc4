"""cineflow.validate on the device: the committed seeded task (tests/golden/plan_and_preprocess/seeded/preprocessed) validated by seeded
tiny networks, a 2-D one on the `_2D_stage0` folder and a 3-D one on `_stage0`, two folds each.

Per case the label file's voxels, the stored softmax and the .pkl equal what the existing host route writes from the same network
(trainer.predict_preprocessed_data_return_seg_and_softmax -> transpose -> export.save_segmentation_nifti_from_softmax with
resampled_npz_fname and properties_pkl=True): the host route's network run is held to the softmax the command exported (equal for the 3-D
network; the 2-D network is not reproducible bit for bit from run to run, RERUN_BAR), and its exporter, fed that softmax, must write
the same three files bit for bit.  Per folder summary.json's results equal aggregate_scores on the written files,
postprocessing.json equals determine_postprocessing run by the file route on a copy, and consolidate_folds runs on the two folds.
Separately, with a second stage folder made here by resizing the cases' data: the pred_next_stage files equal
resample_data_or_seg(...).argmax(0), and a seeded cascade folder takes them back as input."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDED = os.path.join(HERE, "golden", "plan_and_preprocess", "seeded")
STAGES = {"2d": "nnUNetData_plans_v2.1_2D_stage0", "3d": "nnUNetData_plans_v2.1_stage0"}
PLANS_PKL = {"2d": "nnUNetPlansv2.1_plans_2D.pkl", "3d": "nnUNetPlansv2.1_plans_3D.pkl"}
# six cases are too few for KFold(5) over pairs: two folds, the two frames of a patient kept together
FOLDS = [["patientA_f01", "patientA_f02", "patientC_f01", "patientC_f02"], ["patientB_f01", "patientB_f02"]]
CASES = sorted(c for f in FOLDS for c in f)
K = 3                                                                    # the task's plans: num_classes 2, plus background
TF, TB = [2, 0, 1], [1, 2, 0]
VAL = "validation_raw"


def plans_of(kind, prev_stage_classes=None):
    p = {"num_modalities": 2, "num_classes": K, "transpose_forward": TF, "transpose_backward": TB}
    if kind == "2d":                                                     # plans_per_stage[0] of the 2-D plans: patch 40 x 40, three poolings
        p.update(patch_size=[40, 40], mirror_axes=[0, 1], seg_net={"base_num_features": 8, "num_pool": 3, "pool_op_kernel_sizes": [[2, 2]] * 3})
    else:                                                                # ... of the 3-D plans: patch 12 x 40 x 40
        p.update(patch_size=[12, 40, 40], mirror_axes=[0, 1, 2],
                 seg_net={"dim": 3, "base_num_features": 8, "num_pool": 3, "pool_op_kernel_sizes": [[1, 2, 2], [1, 2, 2], [2, 2, 2]],
                          "conv_kernel_sizes": [[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3]]})
        if prev_stage_classes is not None:
            p["seg_net"]["prev_stage_classes"] = prev_stage_classes
    return p


def save_seeded_model(folder, plans, dev, seeds):
    from cineflow import predict as P
    from cineflow.weights import seeded_state_dict
    shapes = P.CineTrainer(plans, dev).seg_net.state_shapes()
    for fold, seed in enumerate(seeds):
        P.save_model_folder(folder, None, None, plans, fold=fold, seg_sd=seeded_state_dict(shapes, seed))
    return folder


def load_fold(model, fold, dev):
    from cineflow.predict import load_model_and_checkpoint_files
    trainer, params = load_model_and_checkpoint_files(model, [fold], device=dev)
    trainer.load_checkpoint_ram(params[0])
    return trainer


def case_data(stage, case):
    from cineflow.safe_pickle import load_plain_pickle
    return np.load(os.path.join(stage, case + ".npz"))["data"], load_plain_pickle(os.path.join(stage, case + ".pkl"))


def same_value(a, b):
    """equal property dicts: same keys, arrays equal in dtype, shape and value, containers element by element"""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def same_json(a, b):
    """equal documents, NaN equal to NaN"""
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    """the seeded task in a tmp dir, with a two-fold splits_final.pkl next to its stage folders"""
    root = tmp_path_factory.mktemp("validate_task")
    pre = str(root / "preprocessed")
    shutil.copytree(os.path.join(SEEDED, "preprocessed"), pre)
    splits = [{"train": np.array(sorted(set(CASES) - set(val))), "val": np.array(val)} for val in FOLDS]
    with open(os.path.join(pre, "splits_final.pkl"), "wb") as f:
        pickle.dump(splits, f)
    return pre, os.path.join(SEEDED, "raw", "labelsTr")


@pytest.fixture(scope="module")
def experiments(dev, task, tmp_path_factory):
    """{kind: (model folder, stage folder, EXPERIMENT, {(fold, case): the softmax the run exported})} after `python -m cineflow.validate` on
    both folds.  The softmax of every case is recorded as the command's own trainer returns it (a host copy of the device tensor), so
    that the host route can be fed the very same numbers: two runs of the 2-D network are not equal bit for bit on the device (see
    test_case_files_equal_the_host_route), two exports of one softmax must be."""
    from cineflow import validate as V
    from cineflow.trainer import CineTrainer
    pre, gt = task
    root = tmp_path_factory.mktemp("validate_out")
    real = CineTrainer.predict_preprocessed_data_return_seg_and_softmax
    log = []

    def recording(self, data, *args, **kwargs):
        res = real(self, data, *args, **kwargs)
        if kwargs.get("return_device"):
            log.append(res[1].contiguous().cpu().numpy())
        return res

    out = {}
    patch = pytest.MonkeyPatch()
    patch.setattr(CineTrainer, "predict_preprocessed_data_return_seg_and_softmax", recording)
    try:
        for kind, seeds in (("2d", (10, 20)), ("3d", (30, 40))):
            model = save_seeded_model(str(root / ("model_" + kind)), plans_of(kind), dev, seeds)
            stage, exp = os.path.join(pre, STAGES[kind]), str(root / ("exp_" + kind))
            del log[:]
            folders = V.main(["-m", model, "--data", stage, "-gt", gt, "-o", exp, "--plans", os.path.join(pre, PLANS_PKL[kind]), "-t", "Task501_SeededCine"])
            assert folders == [os.path.join(exp, "fold_%d" % f, VAL) for f in (0, 1)]
            order = [(fold, case) for fold, val in enumerate(FOLDS) for case in sorted(val)]       # folds in turn, a fold's cases sorted
            assert len(log) == len(order), "one prediction per validation case"
            out[kind] = (model, stage, exp, dict(zip(order, list(log))))
    finally:
        patch.undo()
    return out


def test_some_validation_case_was_resampled(task):
    """a condition of this file: without a case whose stage shape differs from its size before resampling, the resampling branch of the
    one-visit export would go unchecked"""
    pre, _gt = task
    resampled = []
    for kind in STAGES:
        for case in CASES:
            data, props = case_data(os.path.join(pre, STAGES[kind]), case)
            if tuple(np.array(data.shape[1:])[TB]) != tuple(props["size_after_cropping"]):
                resampled.append((kind, case))
    assert resampled, "no case of the seeded task is resampled"
    assert any(k == "3d" for k, _ in resampled)


# what two runs of the existing host route differ by on the device, measured on patientA_f01 (three runs each): the 3-D network's
# softmax is equal bit for bit; the 2-D network's differs in 86 % of its values by at most 7.2e-7 (8 to 15 of 50544 stored fp16
# values change).  So the files are compared on ONE softmax, and a second run of the network is held to RERUN_BAR: equal for the 3-D
# network, and for the 2-D one 1e-5, an order above the route's own spread and two below the fp16 step 2^-11 of the stored values.
RERUN_BAR = {"2d": 1e-5, "3d": 0.0}


@pytest.mark.parametrize("kind", ["2d", "3d"])
def test_case_files_equal_the_host_route(dev, task, experiments, kind, tmp_path):
    from cineflow import export
    from cineflow.nifti import read_nifti
    from cineflow.safe_pickle import load_plain_pickle
    model, stage, exp, exported = experiments[kind]
    differ_between_folds = 0.0
    for fold, val in enumerate(FOLDS):
        trainer = load_fold(model, fold, dev)
        out = os.path.join(exp, "fold_%d" % fold, VAL)
        assert sorted(f[:-7] for f in os.listdir(out) if f.endswith(".nii.gz")) == sorted(val)
        args = json.load(open(os.path.join(out, "validation_args.json")))
        assert args["do_mirroring"] is True and args["save_softmax"] is True and args["step_size"] == 0.5 and args["validation_folder_name"] == VAL
        for case in val:
            data, props = case_data(stage, case)
            raw = exported[(fold, case)]
            # the network of the host route gives what the command's device route gave
            _seg, rerun = trainer.predict_preprocessed_data_return_seg_and_softmax(data[:-1], do_mirroring=True, step_size=0.5, verbose=False)
            assert rerun.shape == raw.shape == (K,) + tuple(data.shape[1:])
            spread = float(np.abs(rerun.astype(np.float64) - raw.astype(np.float64)).max())
            print("%s fold %d %s: host route's network against the exported softmax: max |diff| %.3e" % (kind, fold, case, spread))
            assert spread <= RERUN_BAR[kind], "%s fold %d %s: %.3e" % (kind, fold, case, spread)
            # and from that softmax the host route writes the same three files
            ref = str(tmp_path / ("%s_%d_%s.nii.gz" % (kind, fold, case)))
            export.save_segmentation_nifti_from_softmax(raw.transpose([0] + [i + 1 for i in TB]), ref, props, 1, None, None, None, ref[:-7] + ".npz",
                                                        None, None, 0, verbose=False, properties_pkl=True)
            got, got_geo = read_nifti(os.path.join(out, case + ".nii.gz"))
            want, want_geo = read_nifti(ref)
            assert got.dtype == np.uint8 and got.shape == tuple(props["original_size_of_raw_data"])
            assert np.array_equal(got, want), "%s fold %d %s: %d label voxels differ" % (kind, fold, case, int((got != want).sum()))
            assert len(np.unique(got)) > 1
            for key in ("itk_spacing", "itk_origin", "itk_direction"):
                assert np.array_equal(np.asarray(got_geo[key]), np.asarray(want_geo[key])), key
            sm, sm_ref = np.load(os.path.join(out, case + ".npz"))["softmax"], np.load(ref[:-7] + ".npz")["softmax"]
            assert sm.dtype == np.float16 and sm.shape == (K,) + tuple(props["size_after_cropping"]) == sm_ref.shape
            assert np.array_equal(sm.view(np.uint16), sm_ref.view(np.uint16)), "%s fold %d %s: stored softmax differs" % (kind, fold, case)
            assert same_value(load_plain_pickle(os.path.join(out, case + ".pkl")), load_plain_pickle(ref[:-7] + ".pkl")), "%s: .pkl differs" % case
            if fold == 0 and case == val[0]:                             # fold X is validated by fold X's weights alone
                other = load_fold(model, 1, dev).predict_preprocessed_data_return_seg_and_softmax(data[:-1], do_mirroring=True, step_size=0.5,
                                                                                                  verbose=False)[1]
                differ_between_folds = float(np.abs(other - raw).max())
    assert differ_between_folds > 1e-3, "both folds predict the same: the fold's own weights would go unchecked"


@pytest.mark.parametrize("kind", ["2d", "3d"])
def test_summary_and_postprocessing_equal_the_file_route(dev, task, experiments, kind, tmp_path):
    from cineflow import evaluation, postprocessing
    from cineflow.reference_models import load_reference_pickle
    _model, stage, exp, _exported = experiments[kind]
    gt = os.path.join(exp, "gt_niftis")
    assert sorted(os.listdir(gt)) == [c + ".nii.gz" for c in CASES]
    assert load_reference_pickle(os.path.join(exp, "plans.pkl"))["num_classes"] == K - 1
    for fold, val in enumerate(FOLDS):
        out = os.path.join(exp, "fold_%d" % fold, VAL)
        doc = json.load(open(os.path.join(out, "summary.json")))
        assert doc["task"] == "Task501_SeededCine" and doc["author"] == "Fabian" and doc["name"] == "exp_%s val tiled True" % kind
        pairs = [(os.path.join(out, c + ".nii.gz"), os.path.join(gt, c + ".nii.gz")) for c in sorted(val)]
        want = evaluation.aggregate_scores(pairs, labels=list(range(K)), num_threads=2)
        assert sorted(doc["results"]["mean"]) == [str(c) for c in range(K)]
        assert same_json(doc["results"], json.loads(json.dumps(want))), "fold %d: summary.json differs from the scores of the written files" % fold
        # determine_postprocessing by the file route, on a copy whose summary.json is scored from the files
        base = tmp_path / ("copy_%d" % fold)
        shutil.copytree(out, str(base / VAL))
        evaluation.aggregate_scores([(os.path.join(str(base / VAL), os.path.basename(t)), r) for t, r in pairs], labels=list(range(K)),
                                    json_output_file=str(base / VAL / "summary.json"), num_threads=2)
        postprocessing.determine_postprocessing(str(base), gt, VAL, final_subf_name=VAL + "_postprocessed", debug=False)
        got_pp = json.load(open(os.path.join(exp, "fold_%d" % fold, "postprocessing.json")))
        assert same_json(got_pp, json.load(open(str(base / "postprocessing.json"))))
        assert sorted(f for f in os.listdir(os.path.join(exp, "fold_%d" % fold, VAL + "_postprocessed")) if f.endswith(".nii.gz")) \
            == [c + ".nii.gz" for c in sorted(val)]


def test_consolidate_folds_runs_on_the_written_experiment(dev, experiments, tmp_path):
    """the chain check: what validate wrote is what cineflow.postprocessing reads"""
    from cineflow import postprocessing
    exp = str(tmp_path / "exp")
    shutil.copytree(experiments["3d"][2], exp)
    postprocessing.consolidate_folds(exp, folds=(0, 1))
    assert "for_which_classes" in json.load(open(os.path.join(exp, "postprocessing.json")))
    assert sorted(f for f in os.listdir(os.path.join(exp, "cv_niftis_postprocessed")) if f.endswith(".nii.gz")) == [c + ".nii.gz" for c in CASES]
    assert sorted(json.load(open(os.path.join(exp, "cv_niftis_raw", "summary.json")))["results"]["mean"]) == [str(c) for c in range(K)]


def test_overwrite_0_keeps_the_files_and_scores_them(dev, task, experiments):
    from cineflow import validate as V
    model, stage, exp, _exported = experiments["2d"]
    out = os.path.join(exp, "fold_1", VAL)
    before = {f: os.path.getmtime(os.path.join(out, f)) for f in os.listdir(out) if f.endswith((".nii.gz", ".npz"))}
    results = json.load(open(os.path.join(out, "summary.json")))["results"]
    V.main(["-m", model, "--data", stage, "-gt", task[1], "-o", exp, "-f", "1", "--overwrite", "0", "--disable_postprocessing", "-t", "Task501_SeededCine"])
    assert before == {f: os.path.getmtime(os.path.join(out, f)) for f in before}
    assert same_json(json.load(open(os.path.join(out, "summary.json")))["results"], results)


@pytest.fixture(scope="module")
def next_stage(task, tmp_path_factory):
    """a second stage folder: every case of the 3-D stage resized (data linear, labels nearest) to a larger grid"""
    pre, _gt = task
    root = tmp_path_factory.mktemp("validate_next")
    stage, nxt = os.path.join(pre, STAGES["3d"]), str(root / "preprocessed" / "stage1")
    os.makedirs(nxt)
    for case in CASES:
        data, _props = case_data(stage, case)
        shape = (data.shape[1] + 2, data.shape[2] + 7, data.shape[3] + 5)
        t = torch.from_numpy(data)[None]
        big = torch.cat([F.interpolate(t[:, :-1], size=shape, mode="trilinear", align_corners=False), F.interpolate(t[:, -1:], size=shape, mode="nearest")], 1)
        np.savez_compressed(os.path.join(nxt, case + ".npz"), data=big[0].numpy().astype(np.float32))
        shutil.copy(os.path.join(stage, case + ".pkl"), os.path.join(nxt, case + ".pkl"))
    shutil.copy(os.path.join(pre, "splits_final.pkl"), str(root / "preprocessed" / "splits_final.pkl"))
    return nxt


def test_next_stage_files_and_the_cascade_that_takes_them(dev, task, experiments, next_stage, tmp_path):
    from cineflow import ops
    from cineflow import validate as V
    from cineflow.nifti import read_nifti
    pre, gt = task
    model, stage, _exp, _exported = experiments["3d"]
    low = str(tmp_path / "exp_lowres")
    V.main(["-m", model, "--data", stage, "-gt", gt, "-o", low, "-f", "1", "--next_stage", next_stage, "--no_softmax", "--disable_postprocessing"])
    assert not [f for f in os.listdir(os.path.join(low, "fold_1", VAL)) if f.endswith((".npz", ".pkl"))]
    trainer = load_fold(model, 1, dev)
    for case in FOLDS[1]:
        data, _props = case_data(stage, case)
        target = np.load(os.path.join(next_stage, case + ".npz"))["data"].shape[1:]
        softmax = trainer.predict_preprocessed_data_return_seg_and_softmax(data[:-1], do_mirroring=True, step_size=0.5, verbose=False)[1]
        want = ops.resample_data_or_seg(softmax, target, False, order=1, do_separate_z=False, order_z=0).argmax(0)
        got = np.load(os.path.join(low, "pred_next_stage", case + "_segFromPrevStage.npz"))["data"]
        assert got.dtype == np.uint8 and got.shape == tuple(target) and np.array_equal(got, want), case
        assert len(np.unique(got)) > 1
    # the cascade stage: two modalities plus the one-hot labels of the previous stage
    cascade = save_seeded_model(str(tmp_path / "model_cascade"), plans_of("3d", prev_stage_classes=[1, 2]), dev, (50, 60))
    full = str(tmp_path / "exp_cascade")
    with pytest.raises(ValueError, match="previous stage"):
        V.main(["-m", cascade, "--data", next_stage, "-gt", gt, "-o", full, "-f", "1", "--disable_postprocessing"])
    V.main(["-m", cascade, "--data", next_stage, "-gt", gt, "-o", full, "-f", "1", "--prev_stage", os.path.join(low, "pred_next_stage"),
            "--disable_postprocessing"])
    for case in FOLDS[1]:
        seg, _geo = read_nifti(os.path.join(full, "fold_1", VAL, case + ".nii.gz"))
        _data, props = case_data(next_stage, case)
        assert seg.dtype == np.uint8 and seg.shape == tuple(props["original_size_of_raw_data"])
        assert np.load(os.path.join(full, "fold_1", VAL, case + ".npz"))["softmax"].shape == (K,) + tuple(props["size_after_cropping"])
    # the network saw the labels: other previous-stage labels, another prediction
    other = str(tmp_path / "other_prev")
    os.makedirs(other)
    for case in FOLDS[1]:
        prev = np.load(os.path.join(low, "pred_next_stage", case + "_segFromPrevStage.npz"))["data"]
        np.savez_compressed(os.path.join(other, case + "_segFromPrevStage.npz"), data=((prev + 1) % 3).astype(np.uint8))
    full2 = str(tmp_path / "exp_cascade_other")
    V.main(["-m", cascade, "--data", next_stage, "-gt", gt, "-o", full2, "-f", "1", "--prev_stage", other, "--disable_postprocessing"])
    assert any(not np.array_equal(np.load(os.path.join(full, "fold_1", VAL, c + ".npz"))["softmax"],
                                  np.load(os.path.join(full2, "fold_1", VAL, c + ".npz"))["softmax"]) for c in FOLDS[1])
    os.remove(os.path.join(other, FOLDS[1][0] + "_segFromPrevStage.npz"))
    with pytest.raises(FileNotFoundError, match=FOLDS[1][0]):
        V.main(["-m", cascade, "--data", next_stage, "-gt", gt, "-o", str(tmp_path / "exp_missing"), "-f", "1", "--prev_stage", other,
                "--disable_postprocessing"])
