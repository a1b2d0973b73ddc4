#!/usr/bin/env python3
"""Generate tests/golden/model_selection/{A,B}.npz (the seeded trees: every model's softmax, the ground truth, the geometry) and {A,B}.json
(what the reference made of them) by RUNNING THE REFERENCE's consolidate_folds, its model_selection/ensemble.py `ensemble()` for every pair
and the result-collection and choice part of figure_out_what_to_submit.main on those trees, in the build container (no GPU needed).

    python tests/golden/make_golden_model_selection.py

The stand-ins are make_golden_postprocessing.py's (SimpleITK on cineflow.nifti, batchgenerators' file helpers -- extended here by load_pickle,
save_pickle and subdirs --, medpy = oracle.metrics.medpy_binary, Pool -> ThreadPool).  figure_out_what_to_submit.main is one function that
starts from global path variables and a task search, so it cannot be called on a tree of ours: its single-model part is run call by call
(get_mean_foreground_dice, foreground_mean, load_json, in main's order), its pair loop by calling `ensemble()` with main's names and
arguments, and its choice part -- the lines from `foreground_dices = list(results.values())` to the end of the task loop, which write
prediction_commands.txt and summary.csv -- is cut out of the imported module's source at generation time and executed on those results,
so the tie rule, the command text and the csv formatting are the reference's own.  Nothing of the reference is stored: only its outputs.

Tree A: 3 models x 2 folds x 3 cases, K = 4, fp16 softmaxes, crops of about [4][6][20][19] at unequal margins (x0 not a multiple of 8, X not
a multiple of 8), every case another shape.  A softmax is the blurred one-hot ground truth plus model-specific seeded noise, quantised to
multiples of 1/16 (every other case of a model also sees a false class-2 object in a corner of the crop), so that many voxels tie exactly
between the top two mean entries (asserted: >= 1 % in every pair) and the first-index rule of the arg-max decides them.  Asserted too: the winner leads the runner-up by more than 1e-6, and it is an ensemble.
Tree B: 2 folds x 2 cases, built so that a single model wins (the other models are much noisier); one model's .npz is fp32 and one case
per fold carries a regions_class_order in its .pkl (which the reference's ensemble() does not read: it passes region_class_order=None).
`build_tree` below writes a tree from the arrays; tests/test_gpu_model_selection.py builds its input with the same function."""
import json
import os
import pickle
import shutil
import sys
import tempfile
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "model_selection")
SPACING = (1.25, 1.25, 8.0)          # itk order (x, y, z)
CLASSES = [1, 2, 3]
K = 4
TRAINER, CASCADE_TRAINER, PLANS = "nnUNetTrainerV2", "nnUNetTrainerV2CascadeFullRes", "nnUNetPlansv2.1"
TASK = "Task901_Seeded"
FOLDS = (0, 1)
# tree -> (models, noise of each model, cases per fold, fp32 models, (crop, full, lo) per case)
TREES = {
    "A": dict(models=["2d", "3d_fullres", "3d_lowres"], noise=[1.2, 1.1, 1.3], fp32=[], regions=[],
              cases=[((4, 6, 20, 19), (6, 24, 27), (1, 2, 3)), ((4, 5, 18, 21), (5, 21, 29), (0, 1, 5)), ((4, 6, 22, 17), (7, 22, 25), (1, 0, 3)),
                     ((4, 4, 20, 23), (6, 25, 23), (2, 4, 0)), ((4, 6, 19, 19), (6, 19, 30), (0, 0, 9)), ((4, 5, 21, 20), (6, 26, 26), (1, 3, 1))]),
    "B": dict(models=["2d", "3d_fullres", "3d_lowres"], noise=[0.15, 1.6, 1.9], fp32=["3d_fullres"], regions=[0, 2],
              cases=[((4, 4, 18, 19), (5, 20, 24), (1, 1, 3)), ((4, 5, 20, 17), (5, 20, 17), (0, 0, 0)), ((4, 4, 17, 21), (6, 19, 26), (1, 2, 5)),
                     ((4, 5, 19, 18), (6, 22, 21), (0, 3, 1))]),
}
REGIONS_ORDER = (1, 2, 3, 1)


def model_name(m):
    return m + "__" + (CASCADE_TRAINER if m == "3d_cascade_fullres" else TRAINER) + "__" + PLANS


def case_name(i):
    return "case_%02d" % i


def fold_of(i, n_cases):
    return 0 if i < n_cases // 2 else 1


# ------------------------------------------------------------------------------------------------ seeded data
def _anatomy(rng, full):
    """nested ellipses labelled 1, 2, 3 around the centre of the volume; the first slice is empty"""
    z, y, x = np.meshgrid(*[np.arange(s) for s in full], indexing="ij")
    lab = np.zeros(full, np.uint8)
    cy, cx = full[1] / 2 + rng.normal(0, 0.5), full[2] / 2 + rng.normal(0, 0.5)
    for c, rad in ((1, 0.36), (2, 0.25), (3, 0.13)):
        lab[((y - cy) / (rad * full[1])) ** 2 + ((x - cx) / (rad * full[2])) ** 2 <= 1.0] = c
    lab[0] = 0
    return lab


def _blur(a):
    out = a.copy()
    for axis in (1, 2):
        out = (np.roll(out, 1, axis) + 2 * out + np.roll(out, -1, axis)) / 4
    return out


def make_tree(tag):
    """-> dict of arrays: gt/<case>, lo/<case>, softmax/<model>/<case>, plus the lists the tree is built from"""
    spec = TREES[tag]
    rng = np.random.default_rng({"A": 4101, "B": 4102}[tag])
    fx = {"models": np.array(spec["models"]), "cases": np.array([case_name(i) for i in range(len(spec["cases"]))]),
          "regions": np.array(spec["regions"], dtype=np.int64)}
    for i, (crop, full, lo) in enumerate(spec["cases"]):
        gt = _anatomy(rng, full)
        fx["gt/" + case_name(i)] = gt
        fx["lo/" + case_name(i)] = np.array(lo)
        inside = gt[lo[0]:lo[0] + crop[1], lo[1]:lo[1] + crop[2], lo[2]:lo[2] + crop[3]]
        for n, (m, noise) in enumerate(zip(spec["models"], spec["noise"])):
            seen = inside.copy()
            if (i + n) % 2 == 0:
                seen[1:3, 0:3, 0:4] = 2                                            # a false object in a corner: postprocessing has something to decide
            onehot = np.stack([_blur((seen == k).astype(np.float64)) for k in range(K)])
            p = onehot + noise * rng.random(onehot.shape)
            p = np.round(16 * p / p.sum(0)) / 16                                   # multiples of 1/16: exact in fp16, and ties are frequent
            fx["softmax/%s/%s" % (m, case_name(i))] = p.astype(np.float32 if m in spec["fp32"] else np.float16)
    return fx


def build_tree(root, fx):
    """Writes the tree of `fx` under root: root/<NAME>/ for every model (plans.pkl, gt_niftis/, fold_X/validation_raw/ with the model's own
    labels, .npz, .pkl and a summary.json that names the classes) and root/gt/ (the ground truth the ensembles are scored against).
    -> ordered [(NAME, folder)]"""
    sys.path.insert(0, os.path.join(REPO, "cardiac-segmentation-optical-flow_amd"))
    from cineflow.nifti import write_nifti
    cases = [str(c) for c in fx["cases"]]
    os.makedirs(os.path.join(root, "gt"))
    for c in cases:
        write_nifti(os.path.join(root, "gt", c + ".nii.gz"), fx["gt/" + c], SPACING)
    out = []
    for m in (str(m) for m in fx["models"]):
        folder = os.path.join(root, model_name(m))
        os.makedirs(os.path.join(folder, "gt_niftis"))
        with open(os.path.join(folder, "plans.pkl"), "wb") as f:
            pickle.dump({"all_classes": list(CLASSES), "num_classes": len(CLASSES)}, f)
        for i, c in enumerate(cases):
            gt, lo, softmax = fx["gt/" + c], [int(v) for v in fx["lo/" + c]], fx["softmax/%s/%s" % (m, c)]
            write_nifti(os.path.join(folder, "gt_niftis", c + ".nii.gz"), gt, SPACING)
            val = os.path.join(folder, "fold_%d" % fold_of(i, len(cases)), "validation_raw")
            os.makedirs(val, exist_ok=True)
            crop = softmax.shape[1:]
            own = np.zeros(gt.shape, np.uint8)
            own[lo[0]:lo[0] + crop[0], lo[1]:lo[1] + crop[1], lo[2]:lo[2] + crop[2]] = softmax.argmax(0)
            write_nifti(os.path.join(val, c + ".nii.gz"), own, SPACING)
            np.savez_compressed(os.path.join(val, c + ".npz"), softmax=softmax)
            props = {"size_after_cropping": tuple(int(v) for v in crop), "original_size_of_raw_data": np.array(gt.shape),
                     "crop_bbox": [[a, a + n] for a, n in zip(lo, crop)], "itk_spacing": SPACING, "itk_origin": (0.0, 0.0, 0.0),
                     "itk_direction": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}
            if i in [int(v) for v in fx["regions"]]:
                props["regions_class_order"] = REGIONS_ORDER
            with open(os.path.join(val, c + ".pkl"), "wb") as f:
                pickle.dump(props, f)
            with open(os.path.join(val, "summary.json"), "w") as f:
                json.dump({"results": {"mean": {str(k): {} for k in CLASSES}}}, f)
        out.append((model_name(m), folder))
    return out


def expected_commands(reference_text, folder_of, out):
    """the reference's prediction_commands.txt -> the text cineflow.model_selection writes for the same choice: the same lines in the same
    order, with this project's two commands (a model is named by its folder; the ensemble's postprocessing.json lies under `out`)"""
    lines = []
    for line in reference_text.splitlines():
        words = line.split()
        if words[0] == "nnUNet_predict":
            assert words[1:5:2] == ["-i", "-o"] and words[5:14:2] == ["-tr", "-ctr", "-m", "-p", "-t"], line
            lines.append("python -m cineflow.predict -i %s -o %s -m %s%s" % (words[2], words[4], folder_of[model_name(words[10])],
                                                                           " -z" if words[-1] == "-z" else ""))
        else:
            assert words[0] == "nnUNet_ensemble", line
            lines.append(" ".join(["python -m cineflow.ensemble_predictions"] + words[1:]).replace("RESULTS_FOLDER", out))
    return "".join(line + "\n" for line in lines)


def expected_csv(reference_csv):
    """the reference's summary.csv with a single model's row named by its full NAME (the reference names it by `-m`)"""
    rows = reference_csv.splitlines()
    return "".join((r if i == 0 or r.startswith("ensemble_") else model_name(r.split(",")[0]) + r[len(r.split(",")[0]):]) + "\n"
                   for i, r in enumerate(rows))


# ------------------------------------------------------------------------------------------------ the reference
def install_reference():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "cardiac-segmentation-optical-flow_amd"))
    import make_golden_postprocessing as MP
    MP.install_reference()
    ops = sys.modules["batchgenerators.utilities.file_and_folder_operations"]

    def load_pickle(file, mode="rb"):
        with open(file, mode) as f:
            return pickle.load(f)                                                  # (files written a few lines above by build_tree)

    def save_pickle(obj, file, mode="wb"):
        with open(file, mode) as f:
            pickle.dump(obj, f)

    def subdirs(folder, join=True, prefix=None, suffix=None, sort=True):
        res = [os.path.join(folder, i) if join else i for i in os.listdir(folder) if os.path.isdir(os.path.join(folder, i))
               and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
        return sorted(res) if sort else res

    ops.load_pickle, ops.save_pickle, ops.subdirs, ops.shutil = load_pickle, save_pickle, subdirs, shutil
    ops.__all__ = list(ops.__all__) + ["load_pickle", "save_pickle", "subdirs", "shutil"]
    from multiprocessing.pool import ThreadPool
    import nnunet.evaluation.add_mean_dice_to_json as ref_add
    import nnunet.evaluation.model_selection.ensemble as ref_ens
    import nnunet.evaluation.model_selection.figure_out_what_to_submit as ref_fig
    import nnunet.postprocessing.consolidate_postprocessing as ref_p
    ref_ens.Pool = ThreadPool
    return ref_add, ref_ens, ref_fig, ref_p


def choice_part(ref_fig):
    """the choice part of figure_out_what_to_submit.main as a code object: from `foreground_dices = ...` to the end of the task loop"""
    import inspect
    lines = inspect.getsource(ref_fig.main).splitlines()
    start = next(i for i, line in enumerate(lines) if line.strip().startswith("foreground_dices = list(results.values())"))
    return compile(textwrap.dedent("\n".join(lines[start:])), "figure_out_what_to_submit.main (choice part)", "exec")


def tie_fraction(a, b):
    mean = np.sort(np.mean((a, b), 0).astype(np.float32), 0)
    return float((mean[-1] == mean[-2]).mean())


def strip(results):
    """`results` of a summary.json with the temporary folder cut off its file names"""
    for case in results["all"]:
        for key in ("test", "reference"):
            case[key] = os.path.basename(case[key])
    return results


def run_tree(tag, refs, report):
    from itertools import combinations
    ref_add, ref_ens, ref_fig, ref_p = refs
    fx = make_tree(tag)
    work = tempfile.mkdtemp()
    try:
        named = build_tree(os.path.join(work, "trained"), fx)
        folder_of = dict(named)
        results_root = os.path.join(work, "results")
        pre = os.path.join(work, "preprocessed")
        shutil.copytree(os.path.join(work, "trained", "gt"), os.path.join(pre, TASK, "gt_segmentations"))
        ref_ens.preprocessing_output_dir, ref_ens.network_training_output_dir = pre, results_root
        ref_fig.network_training_output_dir = results_root
        models = [str(m) for m in fx["models"]]
        cases = [str(c) for c in fx["cases"]]

        # ---- main :143-161, model by model
        results, all_results = {}, {}
        for m in models:
            folder = folder_of[model_name(m)]
            ref_p.consolidate_folds(folder, folds=FOLDS, validation_folder_name="validation_raw")
            summary_file = os.path.join(folder, "cv_niftis_raw", "summary.json")
            results[m] = ref_fig.get_mean_foreground_dice(summary_file)
            ref_add.foreground_mean(summary_file)
            all_results[m] = ref_fig.load_json(summary_file)["results"]["mean"]
        # ---- main :163-187, pair by pair
        golden = {"pairs": {}, "single": {m: float(results[m]) for m in models}, "single_mean": {m: all_results[m] for m in models}}
        for m1, m2 in combinations(models, 2):
            name = "ensemble_" + model_name(m1) + "--" + model_name(m2)
            base = os.path.join(results_root, "ensembles", TASK, name)
            os.makedirs(base)
            ref_ens.ensemble(folder_of[model_name(m1)], folder_of[model_name(m2)], base, TASK, "validation_raw", FOLDS, allow_ensembling=True)
            summary_file = os.path.join(base, "ensembled_raw", "summary.json")
            raw = strip(json.load(open(summary_file))["results"])
            results[name] = ref_fig.get_mean_foreground_dice(summary_file)
            ref_add.foreground_mean(summary_file)
            all_results[name] = ref_fig.load_json(summary_file)["results"]["mean"]
            from cineflow.nifti import read_nifti
            for c in cases:
                fx["ensembled_raw/%s/%s" % (name, c)] = read_nifti(os.path.join(base, "ensembled_raw", c + ".nii.gz"))[0]
                fx["ensembled_postprocessed/%s/%s" % (name, c)] = read_nifti(os.path.join(base, "ensembled_postprocessed", c + ".nii.gz"))[0]
            final = json.load(open(os.path.join(base, "ensembled_postprocessed", "summary.json")))
            copied = json.load(open(os.path.join(results_root, "summary_jsons", "%s__%s.json" % (TASK, name))))
            assert final["experiment_name"] == name and copied == final
            pp = json.load(open(os.path.join(base, "postprocessing.json")))
            golden["pairs"][name] = {"summary_raw": raw, "summary_postprocessed": strip(final["results"]), "postprocessing": pp,
                                     "summary_raw_name": json.load(open(summary_file))["name"]}
            ties = [tie_fraction(fx["softmax/%s/%s" % (m1, c)], fx["softmax/%s/%s" % (m2, c)]) for c in cases]
            if tag == "A":
                assert min(ties) >= 0.01, (name, ties)
            report.append("%s %s: mean foreground Dice %.6f, exact top-two ties %.1f-%.1f %% of the voxels, for_which_classes %s"
                          % (tag, name, results[name], 100 * min(ties), 100 * max(ties), pp["for_which_classes"]))
        # ---- main :189-238, the reference's own lines
        out = os.path.join(work, "out")
        os.makedirs(out)
        scope = dict(ref_fig.__dict__)
        scope.update(results=results, all_results=all_results, id_task_mapping={901: TASK}, t=901, tr=TRAINER, trc=CASCADE_TRAINER, pl=PLANS,
                     disable_postprocessing=False, output_folder=out)
        exec(choice_part(ref_fig), scope)
        golden["best"] = scope["best_model"]
        golden["results"] = {k: float(v) for k, v in results.items()}
        golden["commands"] = open(os.path.join(out, "prediction_commands.txt")).read().replace(results_root, "RESULTS_FOLDER")
        golden["csv"] = open(os.path.join(out, "summary.csv")).read()
        ranked = sorted(results.values())
        assert ranked[-1] - ranked[-2] > 1e-6, ranked
        assert golden["best"].startswith("ensemble") == (tag == "A"), golden["best"]
        report.append("%s: best %s (%.6f, runner-up %.6f); single models %s" % (tag, golden["best"], ranked[-1], ranked[-2], golden["single"]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, tag + ".npz"), **fx)
    with open(os.path.join(OUT, tag + ".json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)


def main():
    refs = install_reference()
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    report = []
    for tag in ("A", "B"):
        run_tree(tag, refs, report)
    with open(os.path.join(HERE, "PIN_REPORT_model_selection.txt"), "w") as f:
        f.write("tests/golden/model_selection/: the reference's consolidate_folds, model_selection/ensemble.py ensemble() and the choice part of\n"
                "figure_out_what_to_submit.main (its own lines, cut from the imported module at generation time) run in place on seeded trees\n"
                "(make_golden_model_selection.py, build container).  SimpleITK, batchgenerators' file helpers and medpy are stand-ins: the label\n"
                "files, the confusion-type values of every summary.json, the postprocessing decisions, the chosen name, prediction_commands.txt\n"
                "and summary.csv are the reference's own; the surface metrics of ensembled_postprocessed/summary.json are\n"
                "oracle.metrics.medpy_binary's restatement -- parity unpinned.  main's task search and global path variables are not run: the\n"
                "single-model part and the pair loop are its calls in its order.  The reference's ensemble() passes region_class_order=None, so\n"
                "tree B's regions .pkl does not change its label files.\n")
        for line in report:
            f.write(line + "\n")
    print("\n".join(report))
    print("wrote", sorted(os.listdir(OUT)), "%.1f KiB" % (sum(os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT)) / 1024))


if __name__ == "__main__":
    main()
