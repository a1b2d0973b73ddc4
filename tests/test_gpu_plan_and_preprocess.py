"""python -m cineflow.plan_and_preprocess on the seeded task of tests/golden/plan_and_preprocess/seeded against the tree the reference's
crop, DatasetAnalyzer, planners and preprocessors wrote there (make_golden_plan_and_preprocess.py): cropped arrays and properties,
fingerprint pickles, plans, stage label channels and class locations are EQUAL; stage image channels are within the bars
tests/test_preprocess.py holds the same device functions to (2e-5 absolute for normalised channels, 1e-4 for a channel left
un-normalised; the task's channels, CT and MRI, are both normalised)."""
import os
import shutil

import numpy as np
import pytest

from _plan_compare import assert_same, relative_paths

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDED = os.path.join(HERE, "golden", "plan_and_preprocess", "seeded")
TASK = "Task501_SeededCine"
TOL_NORMALISED, TOL_UNNORMALISED = 2e-5, 1e-4
CASES = ["patientA_f01", "patientA_f02", "patientB_f01", "patientB_f02", "patientC_f01", "patientC_f02"]
STAGES = ["nnUNetData_plans_v2.1_stage0", "nnUNetData_plans_v2.1_2D_stage0"]
PLANS = ["nnUNetPlansv2.1_plans_3D.pkl", "nnUNetPlansv2.1_plans_2D.pkl"]


def _load(path):
    from cineflow.safe_pickle import load_plain_pickle
    return load_plain_pickle(path)


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """one CLI run shared by the tests below -> (root, raw, cropped, preprocessed)"""
    from cineflow import plan_and_preprocess as PP
    root = str(tmp_path_factory.mktemp("pp"))
    raw = os.path.join(root, "nnUNet_raw_data", TASK)
    cropped = os.path.join(root, "nnUNet_cropped_data", TASK)
    pre = os.path.join(root, "nnUNet_preprocessed", TASK)
    shutil.copytree(os.path.join(SEEDED, "raw"), raw)
    assert PP.main(["--raw", raw, "--cropped", cropped, "--preprocessed", pre, "-tf", "40"]) == 0
    return root, raw, cropped, pre


def test_cropped_cases_equal(run):
    root, raw, cropped, _ = run
    assert sorted(f[:-4] for f in os.listdir(cropped) if f.endswith(".npz")) == CASES
    for c in CASES:
        got, want = np.load(os.path.join(cropped, c + ".npz"))["data"], np.load(os.path.join(SEEDED, "cropped", c + ".npz"))["data"]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), c
        assert_same(relative_paths(_load(os.path.join(cropped, c + ".pkl")), root), _load(os.path.join(SEEDED, "cropped", c + ".pkl")), c)
    # a patient's frames share the union box, and the label files and dataset.json were copied
    a, b = _load(os.path.join(cropped, "patientA_f01.pkl")), _load(os.path.join(cropped, "patientA_f02.pkl"))
    assert a["crop_bbox"] == b["crop_bbox"] and a["size_after_cropping"] == b["size_after_cropping"]
    assert sorted(os.listdir(os.path.join(cropped, "gt_segmentations"))) == [c + ".nii.gz" for c in CASES]
    assert open(os.path.join(cropped, "dataset.json")).read() == open(os.path.join(raw, "dataset.json")).read()


@pytest.mark.parametrize("name", ["dataset_properties.pkl", "intensityproperties.pkl", "props_per_case.pkl"])
def test_fingerprint_equal(run, name):
    root, _, cropped, pre = run
    want = _load(os.path.join(SEEDED, "cropped", name))
    assert_same(relative_paths(_load(os.path.join(cropped, name)), root), want, name)
    if name == "dataset_properties.pkl":
        assert want["intensityproperties"] is not None                                  # a CT modality: the samples were collected
        assert_same(_load(os.path.join(pre, name)), _load(os.path.join(cropped, name)), "copy")


@pytest.mark.parametrize("name", PLANS)
def test_plans_equal_and_feed_the_importers(run, name):
    from cineflow.reference_models import plans_from_reference, plans_from_reference_3d
    root, _, _, pre = run
    got = _load(os.path.join(pre, name))
    assert_same(relative_paths(got, root), _load(os.path.join(SEEDED, "preprocessed", name)), name)
    assert [int(v) for v in got["transpose_forward"]] == [2, 0, 1]
    t = plans_from_reference_3d(got) if name.endswith("3D.pkl") else plans_from_reference(got)
    assert t["transpose_forward"] == [2, 0, 1] and t["normalization_schemes"] == {"0": "CT", "1": "nonCT"}


@pytest.mark.parametrize("stage", STAGES)
def test_stage_folders(run, stage):
    root, _, _, pre = run
    assert sorted(f[:-4] for f in os.listdir(os.path.join(pre, stage)) if f.endswith(".npz")) == CASES
    worst = 0.0
    for c in CASES:
        got, want = np.load(os.path.join(pre, stage, c + ".npz"))["data"], np.load(os.path.join(SEEDED, "preprocessed", stage, c + ".npz"))["data"]
        assert got.dtype == np.float32 and got.shape == want.shape, (c, got.shape, want.shape)
        assert np.array_equal(got[-1], want[-1]), "%s: label channel" % c
        err = float(np.abs(got[:-1].astype(np.float64) - want[:-1]).max())
        worst = max(worst, err)
        gp, wp = _load(os.path.join(pre, stage, c + ".pkl")), _load(os.path.join(SEEDED, "preprocessed", stage, c + ".pkl"))
        assert_same(relative_paths(gp, root), wp, "%s/%s" % (stage, c))
        for k, locs in wp["class_locations"].items():
            if len(locs):
                assert np.array_equal(want[-1][tuple(np.asarray(locs).T)], np.full(len(locs), k, np.float32))
    print("%s: max |image - reference| = %.3e (bar %.0e)" % (stage, worst, TOL_NORMALISED))
    assert worst <= TOL_NORMALISED
    assert _load(os.path.join(SEEDED, "preprocessed", stage, "patientB_f02.pkl"))["class_locations"][2] == []
    assert sorted(os.listdir(os.path.join(pre, "gt_segmentations"))) == [c + ".nii.gz" for c in CASES]


def test_no_pp_writes_plans_and_no_stage_folder(run, tmp_path):
    from cineflow import plan_and_preprocess as PP
    root, raw, cropped, pre = run
    pre2 = str(tmp_path / "nnUNet_preprocessed" / TASK)
    assert PP.main(["--raw", raw, "--cropped", cropped, "--preprocessed", pre2, "-no_pp"]) == 0          # (the cropped cases are there: kept)
    assert sorted(os.listdir(pre2)) == sorted(PLANS + ["dataset.json", "dataset_properties.pkl"])
    for name in PLANS:
        assert_same(relative_paths(relative_paths(_load(os.path.join(pre2, name)), str(tmp_path)), root), _load(os.path.join(SEEDED, "preprocessed", name)), name)
    with pytest.raises(NotImplementedError, match="ExperimentPlanner3D_v21_32"):
        PP.main(["--raw", raw, "--cropped", cropped, "--preprocessed", pre2, "-pl3d", "ExperimentPlanner3D_v21_32", "-no_pp"])
