#!/usr/bin/env python3
"""Generate tests/golden/plan_and_preprocess/ by RUNNING THE REFERENCE's crop, DatasetAnalyzer, experiment planners and preprocessing
drivers on a seeded synthetic task and on planner-only dataset properties, in the build container (no GPU needed).

    python tests/golden/make_golden_plan_and_preprocess.py

The reference is imported in place (_ref_import).  Stand-ins, because the packages are absent from the image:
  * SimpleITK and batchgenerators' file helpers: make_golden_postprocessing.py's (plus load_pickle / save_pickle / subdirs);
  * `resize` / `resize_segmentation` inside nnunet.preprocessing.preprocessing = oracle.preprocess's restatements, as
    make_golden_preprocess.py injects them: parity of those two third-party functions stays unpinned, as it is there;
  * multiprocessing Pool -> ThreadPool of ONE thread in the four reference modules (PreprocessorFor2D.resample_and_normalize writes the
    case's own slice spacing into the target-spacing array all cases share: only a serial run is well defined);
  * nnunet.training.model_restore.recursive_find_python_class (it imports the trainers) = a lookup in nnunet.preprocessing.preprocessing.
The fork's GenericPreprocessor.run does not take the `keep_spacing` its planner passes (ExperimentPlanner.run_preprocessing raises a
TypeError for every 3-D planner), so the 3-D stage folders come from the reference's own GenericPreprocessor._run_internal, called per
case with keep_spacing=False, after the copy of gt_segmentations that run_preprocessing starts with.

Seeded task (Task501_SeededCine): 3 patients x 2 frames, modalities CT and MRI, arrays of 40-46 x 36-42 x 10-12 voxels with ITK spacing
(8 or 7, 1.4, 1.4) -- the coarse axis is the LAST array axis, so transpose_forward is [2, 0, 1] -- a zero frame of another width per
frame (the patient's union box pads), labels 0-2 with class 2 absent from one case.  Planner-only properties (no images): `lowres`
(large isotropic cases: a 3d_lowres stage), `shrink2d` (slices too large for the 2-D budget: the `while here > ref` loop runs) and
`custom` (CustomExperimentPlanner with its YAML).  Every one of these branch conditions is asserted below before anything is written.

Paths inside the stored pickles are made relative to the run's root folder; the test does the same with its own.
"""
import json
import os
import pickle
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "cardiac-segmentation-optical-flow_amd"))

import _ref_import  # noqa: E402
import make_golden_postprocessing as MGP  # noqa: E402

OUT = os.path.join(HERE, "plan_and_preprocess")
ROOT = "/tmp/cineflow_golden_plan_and_preprocess"          # no "28" / "027" in it: the fork's planners look for those in their paths
TASK = "Task501_SeededCine"
CUSTOM_CONFIG = {"batch_size": 6, "in_encoder_dims": [32, 64, 128]}


def relative_paths(obj, root):
    """every string below `root` -> its path relative to root (containers rebuilt, everything else as it is)"""
    if isinstance(obj, str):
        return os.path.relpath(obj, root) if obj.startswith(root) else obj
    if isinstance(obj, dict):
        out = type(obj)()
        for k, v in obj.items():
            out[k] = relative_paths(v, root)
        return out
    if isinstance(obj, (list, tuple)):
        return type(obj)(relative_paths(v, root) for v in obj)
    return obj


def install_reference():
    os.environ["nnUNet_raw_data_base"] = ROOT
    os.environ["nnUNet_preprocessed"] = os.path.join(ROOT, "nnUNet_preprocessed")
    sitk = MGP._sitk_module()
    sitk.Image.GetSize = lambda self: tuple(int(v) for v in self.array.shape[::-1])        # ITK order (x, y, z)
    sys.modules["SimpleITK"] = sitk
    _ref_import.install()
    import batchgenerators.utilities  # noqa: F401
    fo = MGP._file_ops_module()

    def load_pickle(file, mode="rb"):
        with open(file, mode) as f:
            return pickle.load(f)

    def save_pickle(obj, file, mode="wb"):
        with open(file, mode) as f:
            pickle.dump(obj, f)

    def subdirs(folder, join=True, prefix=None, suffix=None, sort=True):
        res = [os.path.join(folder, i) if join else i for i in os.listdir(folder) if os.path.isdir(os.path.join(folder, i))
               and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
        return sorted(res) if sort else res

    fo.pickle, fo.json, fo.load_pickle, fo.save_pickle, fo.subdirs = pickle, json, load_pickle, save_pickle, subdirs
    fo.__all__ = fo.__all__ + ["pickle", "json", "load_pickle", "save_pickle", "subdirs"]
    sys.modules["batchgenerators.utilities.file_and_folder_operations"] = fo

    restore = types.ModuleType("nnunet.training.model_restore")
    restore.recursive_find_python_class = lambda folder, name, current_module: getattr(sys.modules["nnunet.preprocessing.preprocessing"], name, None)
    sys.modules["nnunet.training.model_restore"] = restore

    from multiprocessing.pool import ThreadPool
    from oracle import preprocess as OP
    import nnunet.preprocessing.cropping as ref_crop
    import nnunet.preprocessing.preprocessing as ref_pp
    import nnunet.experiment_planning.DatasetAnalyzer as ref_da
    import nnunet.experiment_planning.utils as ref_utils
    ref_pp.resize, ref_pp.resize_segmentation = OP.resize, OP.resize_segmentation
    for m in (ref_crop, ref_pp, ref_da, ref_utils):
        m.Pool = lambda n=None: ThreadPool(1)
    return ref_utils, ref_da, ref_pp


# ------------------------------------------------------------------------------------------------ the seeded task
def build_task(folder):
    from cineflow.nifti import write_nifti
    rng = np.random.default_rng(501)
    os.makedirs(os.path.join(folder, "imagesTr"))
    os.makedirs(os.path.join(folder, "labelsTr"))
    training = []
    # patient: array shape (the coarse axis last), slice spacing; per frame the widths of the zero frame (lo, hi) per array axis
    patients = [("patientA", (44, 40, 12), 8.0, [((3, 2), (2, 4), (1, 0)), ((5, 3), (3, 2), (0, 1))]),
                ("patientB", (40, 36, 10), 8.0, [((2, 2), (1, 1), (0, 0)), ((2, 4), (3, 1), (0, 0))]),
                ("patientC", (46, 42, 11), 7.0, [((4, 1), (2, 2), (1, 1)), ((1, 5), (4, 3), (0, 1))])]
    for name, shape, dz, frames in patients:
        for f, frame in enumerate(frames):
            case = "%s_f%02d" % (name, f + 1)
            box = tuple(slice(lo, n - hi) for (lo, hi), n in zip(frame, shape))
            g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
            r = np.sqrt(g[0] ** 2 + g[1] ** 2 + 0.2 * g[2] ** 2)
            lab = np.zeros(shape, np.uint8)
            lab[r < 0.55] = 1
            if case != "patientB_f02":                         # class 2 is absent from this one case
                lab[r < 0.3] = 2
            keep = np.zeros(shape, bool)
            keep[box] = True
            lab[~keep] = 0
            for m, (mean, sd) in enumerate(((60.0, 40.0), (400.0, 120.0))):
                img = np.round(rng.normal(size=shape) * sd + mean + 80.0 * (lab > 0)).astype(np.float32)
                img[img == 0] = 1.0
                img[~keep] = 0.0
                write_nifti(os.path.join(folder, "imagesTr", "%s_%04d.nii.gz" % (case, m)), img, (dz, 1.4, 1.4), (0.0, 0.0, 0.0))
            write_nifti(os.path.join(folder, "labelsTr", case + ".nii.gz"), lab, (dz, 1.4, 1.4), (0.0, 0.0, 0.0))
            training.append({"image": "./imagesTr/%s.nii.gz" % case, "label": "./labelsTr/%s.nii.gz" % case, "center": "c%d" % (f + 1),
                             "phase": "ED" if f == 0 else "ES"})
    with open(os.path.join(folder, "dataset.json"), "w") as fh:
        json.dump({"name": "SeededCine", "modality": {"0": "CT", "1": "MRI"}, "labels": {"0": "background", "1": "ring", "2": "core"},
                   "numTraining": len(training), "training": training, "test": []}, fh, indent=1)


def run_seeded(ref_utils, ref_da, ref_pp):
    from nnunet.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
    from nnunet.experiment_planning.experiment_planner_baseline_2DUNet_v21 import ExperimentPlanner2D_v21
    raw = os.path.join(ROOT, "nnUNet_raw_data", TASK)
    cropped = os.path.join(ROOT, "nnUNet_cropped_data", TASK)
    pre = os.path.join(ROOT, "nnUNet_preprocessed", TASK)
    build_task(raw)
    ref_utils.crop(TASK, False, 1)
    an = ref_da.DatasetAnalyzer(cropped, overwrite=False, num_processes=1)
    props = an.analyze_dataset(True)
    an.analyse_segmentations()
    os.makedirs(pre)
    shutil.copy(os.path.join(cropped, "dataset_properties.pkl"), pre)

    # ---- the branch conditions the fixture is there for
    cases = sorted(f[:-4] for f in os.listdir(cropped) if f.endswith(".npz"))
    assert len(cases) == 6
    raw_boxes = {}
    for c in cases:
        with open(os.path.join(cropped, c + ".pkl"), "rb") as f:
            p = pickle.load(f)
        full = np.load(os.path.join(cropped, c + ".npz"))["data"]
        assert tuple(full.shape[1:]) == tuple(p["size_after_cropping"]) and full.shape[0] == 3
        raw_boxes[c] = (p, full)
    for name in ("patientA", "patientB", "patientC"):
        a, b = raw_boxes[name + "_f01"], raw_boxes[name + "_f02"]
        assert a[1].shape == b[1].shape and a[0]["crop_bbox"] == b[0]["crop_bbox"]
        # the union box pads: some border plane of one frame is all zero in the images although the box was cropped to non-zero
        planes = [np.abs(x[1][:2]).sum(axis=tuple(i for i in range(4) if i != ax + 1)) for x in (a, b) for ax in range(3)]
        assert any(pl[0] == 0 or pl[-1] == 0 for pl in planes), name
    assert props["intensityproperties"] is not None and set(props["modalities"].values()) == {"CT", "MRI"}
    assert 2.0 not in np.unique(raw_boxes["patientB_f02"][1][-1]) and 2.0 in np.unique(raw_boxes["patientB_f01"][1][-1])

    p3 = ExperimentPlanner3D_v21(cropped, pre)
    p3.plan_experiment()
    spac = np.vstack(props["all_spacings"])
    assert list(p3.transpose_forward) == [2, 0, 1]
    assert p3.plans["plans_per_stage"][0]["current_spacing"][0] != np.median(spac[:, 2]), "the anisotropic target-spacing rule did not act"
    assert p3.plans["num_stages"] == 1
    gt = os.path.join(pre, "gt_segmentations")
    shutil.copytree(os.path.join(cropped, "gt_segmentations"), gt)
    pp = ref_pp.GenericPreprocessor(p3.plans["normalization_schemes"], p3.plans["use_mask_for_norm"], p3.transpose_forward,
                                    p3.plans["dataset_properties"]["intensityproperties"])
    assert p3.plans["normalization_schemes"][0] == "CT" and p3.plans["normalization_schemes"][1] == "nonCT"
    for k, stage in p3.plans["plans_per_stage"].items():
        folder = os.path.join(pre, p3.plans["data_identifier"] + "_stage%d" % k)
        os.makedirs(folder)
        for c in cases:
            pp._run_internal(stage["current_spacing"], c, folder, cropped, None, props["all_classes"], False)
    p2 = ExperimentPlanner2D_v21(cropped, pre)
    p2.plan_experiment()
    p2.run_preprocessing((1, 1))
    locs = pickle.load(open(os.path.join(pre, p2.plans["data_identifier"] + "_stage0", "patientB_f02.pkl"), "rb"))["class_locations"]
    assert locs[2] == [] and len(locs[1]) > 0
    return raw, cropped, pre


def store_seeded(raw, cropped, pre):
    dst = os.path.join(OUT, "seeded")
    shutil.copytree(raw, os.path.join(dst, "raw"))
    for src, name in ((cropped, "cropped"), (pre, "preprocessed")):
        for dirpath, dirnames, filenames in os.walk(src):
            if os.path.basename(dirpath) == "gt_segmentations":
                continue
            rel = os.path.relpath(dirpath, src)
            os.makedirs(os.path.join(dst, name, rel), exist_ok=True)
            for fn in filenames:
                s, d = os.path.join(dirpath, fn), os.path.join(dst, name, rel, fn)
                if fn.endswith(".pkl"):
                    with open(s, "rb") as f:
                        obj = relative_paths(pickle.load(f), ROOT)
                    with open(d, "wb") as f:
                        pickle.dump(obj, f, protocol=4)
                elif fn.endswith(".npz"):
                    shutil.copy(s, d)                          # (dataset.json copies are not stored: the raw one is)


# ------------------------------------------------------------------------------------------------ planner-only properties
def planner_only_sets():
    rng = np.random.default_rng(77)

    def props(sizes, spacings, modalities, classes, reduction):
        cases = ["case%02d" % i for i in range(len(sizes))]
        return {"all_sizes": [tuple(int(v) for v in s) for s in sizes], "all_spacings": [np.array(s, dtype=np.float64) for s in spacings],
                "all_classes": classes, "modalities": modalities, "intensityproperties": None,
                "size_reductions": {c: float(reduction) for c in cases}}, cases

    lowres = props(rng.integers(380, 460, size=(7, 3)), 0.8 + 0.1 * rng.random((7, 3)), {0: "CT"}, [1, 2, 3], 1.0)
    shrink = props(np.stack([rng.integers(9, 13, 5), rng.integers(1400, 1600, 5), rng.integers(1400, 1600, 5)], 1),
                   np.stack([np.full(5, 6.0), 0.5 + 0.02 * rng.random(5), 0.5 + 0.02 * rng.random(5)], 1), {0: "MRI"}, [1, 2], 0.6)
    custom = props(np.stack([rng.integers(8, 12, 8), rng.integers(200, 260, 8), rng.integers(190, 250, 8)], 1),
                   np.stack([np.full(8, 10.0), 1.25 + 0.3 * rng.random(8), 1.25 + 0.3 * rng.random(8)], 1), {0: "MRI"}, [1, 2, 3], 0.9)
    return {"lowres": (lowres, ["ExperimentPlanner", "ExperimentPlanner3D_v21", "ExperimentPlanner2D", "ExperimentPlanner2D_v21"]),
            "shrink2d": (shrink, ["ExperimentPlanner3D_v21", "ExperimentPlanner2D_v21"]),
            "custom": (custom, ["CustomExperimentPlanner", "ExperimentPlanner2D", "ExperimentPlanner2D_v21", "ExperimentPlanner", "ExperimentPlanner3D_v21"])}


def make_planner_folder(root, name, props, cases):
    """a cropped folder as far as a planner reads it: dataset_properties.pkl, the case list (.npz names) and each case's .pkl"""
    cropped, pre = os.path.join(root, "cropped_" + name), os.path.join(root, "planned_" + name)
    os.makedirs(cropped)
    os.makedirs(pre)
    with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
        pickle.dump(props, f)
    for c in cases:
        open(os.path.join(cropped, c + ".npz"), "wb").close()
        with open(os.path.join(cropped, c + ".pkl"), "wb") as f:
            pickle.dump({}, f)
    return cropped, pre


def run_planner_only():
    import yaml
    from nnunet.experiment_planning.experiment_planner_baseline_3DUNet import ExperimentPlanner
    from nnunet.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
    from nnunet.experiment_planning.experiment_planner_baseline_2DUNet import ExperimentPlanner2D
    from nnunet.experiment_planning.experiment_planner_baseline_2DUNet_v21 import ExperimentPlanner2D_v21
    import nnunet.experiment_planning.experiment_planner_baseline_2DUNet_v21 as v21_module
    from nnunet.experiment_planning.custom_experiment_planner import CustomExperimentPlanner
    from nnunet.experiment_planning.common_utils import pad_shape
    classes = {c.__name__: c for c in (ExperimentPlanner, ExperimentPlanner3D_v21, ExperimentPlanner2D, ExperimentPlanner2D_v21, CustomExperimentPlanner)}
    if not hasattr(v21_module, "deepcopy"):                   # (the module uses deepcopy in its loop without importing it)
        from copy import deepcopy
        v21_module.deepcopy = deepcopy
    cwd = os.path.join(ROOT, "cwd")
    os.makedirs(cwd)
    with open(os.path.join(cwd, "adversarial_acdc.yaml"), "w") as f:
        yaml.safe_dump(CUSTOM_CONFIG, f)
    os.chdir(cwd)
    out = {}
    for name, ((props, cases), planners) in planner_only_sets().items():
        cropped, pre = make_planner_folder(ROOT, name, props, cases)
        plans = {}
        for pl in planners:
            p = classes[pl](cropped, pre)
            p.plan_experiment()
            with open(p.plans_fname, "rb") as f:
                plans[pl] = relative_paths(pickle.load(f), ROOT)
        with open(os.path.join(cropped, cases[0] + ".pkl"), "rb") as f:
            case_pkl = pickle.load(f)
        out[name] = {"dataset_properties": props, "cases": cases, "plans": plans, "case_pkl": case_pkl}
    # ---- branch conditions
    assert out["lowres"]["plans"]["ExperimentPlanner3D_v21"]["num_stages"] == 2 and out["lowres"]["plans"]["ExperimentPlanner"]["num_stages"] == 2
    st = out["shrink2d"]["plans"]["ExperimentPlanner2D_v21"]["plans_per_stage"][0]
    padded = pad_shape(st["median_patient_size_in_voxels"][1:], 2 ** np.array(st["num_pool_per_axis"]))
    assert np.any(np.array(st["patch_size"]) < padded), "the 2-D `while here > ref` loop did not run"
    assert out["shrink2d"]["case_pkl"]["use_nonzero_mask_for_norm"][0] is True
    cu = out["custom"]["plans"]["CustomExperimentPlanner"]
    assert cu["data_identifier"] == "custom_experiment_planner" and list(cu["plans_per_stage"][0]["patch_size"]) == [288, 288]
    assert cu["plans_per_stage"][0]["batch_size"] == CUSTOM_CONFIG["batch_size"]
    out["custom"]["config"] = CUSTOM_CONFIG
    return out


def main():
    assert "28" not in ROOT and "027" not in ROOT
    for d in (ROOT, OUT):
        if os.path.isdir(d):
            shutil.rmtree(d)
    os.makedirs(ROOT)
    os.makedirs(OUT)
    ref_utils, ref_da, ref_pp = install_reference()
    store_seeded(*run_seeded(ref_utils, ref_da, ref_pp))
    with open(os.path.join(OUT, "planner_only.pkl"), "wb") as f:
        pickle.dump(run_planner_only(), f, protocol=4)
    total = 0
    for dirpath, _, filenames in os.walk(OUT):
        for fn in filenames:
            size = os.path.getsize(os.path.join(dirpath, fn))
            total += size
            assert size < 1 << 20, (fn, size)
    print("wrote %s: %.1f KiB" % (OUT, total / 1024))


if __name__ == "__main__":
    main()
