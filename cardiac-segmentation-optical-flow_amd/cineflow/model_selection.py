"""nnUNet_find_best_configuration on the HIP path: which trained model, or which pair of them, predicts the test set.

Mirrors `nnunet/evaluation/model_selection/figure_out_what_to_submit.py` (`get_foreground_mean` :41, `get_mean_foreground_dice` :36, the loop
of `main` :94-238 as `find_best_configuration`) and `nnunet/evaluation/model_selection/ensemble.py` (`ensemble` :39-123, same folder checks
and AssertionError texts, same skip-if-present rules).  The reference reads its folders from global path variables; here every path is an
argument:

    python -m cineflow.model_selection -m NAME=FOLDER [NAME=FOLDER ...] -gt GT_NIFTIS -o OUT
           [-val validation_raw] [-f 0 1 2 3 4] [-t TASK_NAME] [--disable_ensembling] [--disable_postprocessing]

FOLDER is a trainer output folder (plans.pkl, gt_niftis/, fold_X/<val>/ with *.nii.gz, *.npz, *.pkl and summary.json), NAME the reference's
`<model>__<trainer>__<plans>` string, used verbatim in `ensemble_<NAME1>--<NAME2>`.  A model's own score comes from its cv_niftis_raw
summary (cineflow.postprocessing.consolidate_folds, or collect_cv_niftis + evaluate_folder with --disable_postprocessing, made when absent).

The pairs are where the reference spends its time: for each of the M (M - 1) / 2 pairs it inflates both members' .npz of every validation
case, writes the label file, and reads it back to score it.  Here a validation case is visited once: every member and the ground truth
are uploaded once and ONE `cineflow.ops.ensemble_pairs` launch gives the label volume of every pair and its 16 x 16 label confusion against
the ground truth; `ensembled_raw/summary.json` is aggregate_scores' document built from those counts (`evaluation.Counted`), so no label
file is read back.  A case whose confusion has voxels in the overflow bin (a label >= 16) is scored from its written file instead.
`determine_postprocessing` then runs unchanged on each pair's folder.

Differences that are deliberate:
  * members of one case with different dtypes (one model saved float32) are widened to float32 on the host: exact, and numpy's own
    result type for `np.mean((a, b), 0)`;
  * the reference's merge passes region_class_order=None to the export whatever the .pkl says, i.e. it takes the arg-max of a region
    model's sigmoid maps; that is the default here too (the choice must be the reference's), and --regions_class_order_from_pkl applies
    the order recorded in the first member's .pkl, as cineflow.ensemble_predictions does;
  * the commands of prediction_commands.txt are this project's: `python -m cineflow.predict ... -m FOLDER [-z]` and
    `python -m cineflow.ensemble_predictions -f ... -o ... [-pp <that ensemble's postprocessing.json>]` stand where the reference prints
    nnUNet_predict -tr/-ctr/-m/-p/-t and nnUNet_ensemble; the lines, their order and the tie rule are the reference's;
  * a single model is keyed by its full NAME in the results and in summary.csv (the reference keys it by `-m`, which two trainers of one
    configuration would share);
  * pickles go through the safe unpicklers; the pair's identifier lists must also be equally long (the reference compares them zipped)."""
import argparse
import os
import shutil
from collections import OrderedDict
from itertools import combinations
from os.path import isdir, isfile, join

import numpy as np

from .evaluation import Counted, HIST_K, aggregate_scores, evaluate_folder
from .folder_io import load_json, load_softmax, load_volume, save_json, softmax_case_geometry, subfiles
from .metrics import label_volume_u8
from .nifti import write_nifti
from .postprocessing import collect_cv_niftis, consolidate_folds, determine_postprocessing
from .reference_models import load_reference_pickle
from .safe_pickle import load_plain_pickle

default_num_threads = 8
RERUN = "Please rerun validation with `nnUNet_train CONFIG TRAINER TASK FOLD -val --npz`"


def get_foreground_mean(results):
    results_mean = results["results"]["mean"]
    dice_scores = [results_mean[i]["Dice"] for i in results_mean.keys() if i != "0" and i != "mean"]
    return np.mean(dice_scores)


def get_mean_foreground_dice(json_file):
    return get_foreground_mean(load_json(json_file))


def foreground_mean(filename):
    """nnunet/evaluation/add_mean_dice_to_json.py:21-39: adds results/mean/mean = the nanmean over the foreground classes of every metric
    (classes 0, -1 and 99 do not count; an entry '99' is dropped) and rewrites the file."""
    res = load_json(filename)
    mean = res["results"]["mean"]
    class_ids = [int(i) for i in mean.keys() if i != "mean"]
    class_ids = [i for i in class_ids if i not in (0, -1, 99)]
    mean.pop("99", None)
    metrics = list(mean["1"].keys())
    mean["mean"] = OrderedDict((m, np.nanmean([mean[str(i)][m] for i in class_ids])) for m in metrics)
    save_json(res, filename)


def ensemble_name(name1, name2):
    return "ensemble_" + name1 + "--" + name2


def _validation_cases(folder1, folder2, validation_folder, folds):
    """ensemble.py:58-97 for one pair of training output folders -> [(fold, case identifier)] in the reference's order"""
    cases = []
    for f in folds:
        net1 = join(folder1, "fold_%d" % f, validation_folder)
        net2 = join(folder2, "fold_%d" % f, validation_folder)
        if not isdir(net1):
            raise AssertionError("Validation directory missing: %s. %s" % (net1, RERUN))
        if not isdir(net2):
            raise AssertionError("Validation directory missing: %s. %s" % (net2, RERUN))
        if not isfile(join(net1, "summary.json")):
            raise AssertionError("Validation directory incomplete: %s. %s" % (net1, RERUN))
        if not isfile(join(net2, "summary.json")):
            raise AssertionError("Validation directory missing: %s. %s" % (net2, RERUN))
        ids_npz, ids_nii = [], []
        for net in (net1, net2):
            ids_npz.append([i[:-4] for i in subfiles(net, suffix="npz", join_=False)])
            ids_nii.append([i[:-7] for i in subfiles(net, suffix="nii.gz", join_=False)
                            if not i.endswith("noPostProcess.nii.gz") and not i.endswith("_postprocessed.nii.gz")])
        for net, npz, nii in zip((net1, net2), ids_npz, ids_nii):
            if not all(i in npz for i in nii):
                raise AssertionError("Missing npz files in folder %s. Please run the validation for all models and folds with the '--npz' flag."
                                     % net)
        ids_npz[0].sort()
        ids_npz[1].sort()
        assert len(ids_npz[0]) == len(ids_npz[1]) and all(i == j for i, j in zip(*ids_npz)), "npz filenames do not match. This should not happen."
        cases.extend((f, p) for p in ids_npz[0])
    return cases


def _visit_case(folders, wanted, fold, case, validation_folder, gt_file, regions_from_pkl):
    """One validation case, one launch: wanted = [(a, b)] indices into `folders` -> {(a, b): (labels uint8 [Zf,Yf,Xf] numpy, hist [257]
    numpy, props of member a)}.  Pairs are grouped by what the launch shares: the first member's geometry and region order."""
    import torch
    from . import ops
    used = sorted(set(i for ab in wanted for i in ab))
    assert len(used) >= 2, "a pair needs two members"
    val = {i: join(folders[i], "fold_%d" % fold, validation_folder) for i in used}
    softmax = {i: load_softmax(join(val[i], case + ".npz")) for i in used}           # each model's .npz is inflated once
    props = {i: load_plain_pickle(join(val[i], case + ".pkl")) for i in set(a for a, _ in wanted)}
    shapes = {softmax[i].shape for i in used}
    if len(shapes) != 1:
        raise ValueError("%s: the models' softmax shapes differ: %s" % (case, sorted(shapes)))
    dtypes = {softmax[i].dtype for i in used}
    if not dtypes <= {np.dtype(np.float16), np.dtype(np.float32)}:
        raise ValueError("%s: softmax must be float16 or float32, got %s" % (case, sorted(str(d) for d in dtypes)))
    if len(dtypes) > 1:                                                                 # np.mean((a, b), 0)'s own result type; exact
        softmax = {i: s.astype(np.float32) for i, s in softmax.items()}
    dev = torch.device("cuda", torch.cuda.current_device())
    members = [torch.from_numpy(np.ascontiguousarray(softmax[i])).to(dev) for i in used]     # each member is uploaded once
    gt = label_volume_u8(load_volume(gt_file).array, gt_file)                                  # and the ground truth once
    slot = {i: n for n, i in enumerate(used)}
    groups = OrderedDict()
    for a, b in wanted:
        full, lo = softmax_case_geometry(softmax[a].shape, props[a], join(val[a], case))
        order = props[a].get("regions_class_order") if regions_from_pkl else None
        groups.setdefault((full, lo, None if order is None else tuple(order)), []).append((a, b))
    out = {}
    for (full, lo, order), pairs in groups.items():                                     # one group, unless the first members' .pkl disagree
        if tuple(gt.shape) != full:
            raise ValueError("%s: the ground truth is %s, the case's original size is %s" % (gt_file, tuple(gt.shape), full))
        seg, hist = ops.ensemble_pairs(members, [(slot[a], slot[b]) for a, b in pairs], gt, lo, regions_class_order=order)
        seg, hist = seg.cpu().numpy(), hist.cpu().numpy()
        for n, ab in enumerate(pairs):
            out[ab] = (seg[n], hist[n], props[ab[0]])
    return out


def _ensemble_pairs(folders, wanted, bases, task, validation_folder, folds, gt_folder, allow_ensembling, regions_from_pkl, out_dir_all_json):
    """ensemble.py:39-123 for every (a, b) of `wanted` at once (bases[(a, b)]: that pair's output_folder_base; out_dir_all_json: where the
    postprocessed summaries are gathered)"""
    plans = load_reference_pickle(join(folders[wanted[0][0]], "plans.pkl"))             # only for the labels
    cases = {ab: _validation_cases(folders[ab[0]], folders[ab[1]], validation_folder, folds) for ab in wanted}
    for ab in wanted:
        print("\nEnsembling folders\n", folders[ab[0]], "\n", folders[ab[1]])
        os.makedirs(join(bases[ab], "ensembled_raw"), exist_ok=True)
    out_file = lambda ab, case: join(bases[ab], "ensembled_raw", case + ".nii.gz")       # noqa: E731
    visits = OrderedDict()                                                               # (fold, case) -> the pairs that still lack its file
    for ab in wanted:
        for fc in cases[ab]:
            if not isfile(out_file(ab, fc[1])):
                visits.setdefault(fc, []).append(ab)
    counted = {ab: {} for ab in wanted}
    in_histogram = all(0 <= int(c) < HIST_K for c in plans["all_classes"])               # else every case is scored from its file
    for (fold, case), todo in visits.items():
        gt_file = join(gt_folder, case + ".nii.gz")
        for ab, (seg, hist, props) in _visit_case(folders, todo, fold, case, validation_folder, gt_file, regions_from_pkl).items():
            write_nifti(out_file(ab, case), seg, props["itk_spacing"], props["itk_origin"], props["itk_direction"])
            if not hist[-1] and in_histogram:                                            # every voxel of both volumes is below 16
                counted[ab][case] = Counted(out_file(ab, case), hist[:-1].reshape(HIST_K, HIST_K), int(seg.size))

    for ab in wanted:
        base = bases[ab]
        folder = join(base, "ensembled_raw")
        name = os.path.basename(os.path.normpath(base))
        if not isfile(join(folder, "summary.json")) and len(cases[ab]) > 0:
            # a case written by this run brings its counts; one that was already there (or overflowed) is scored from its file
            pairs = [(counted[ab].get(case, out_file(ab, case)), join(gt_folder, case + ".nii.gz")) for _, case in cases[ab]]
            aggregate_scores(pairs, labels=plans["all_classes"], json_output_file=join(folder, "summary.json"), json_task=task,
                             json_name=task + "__" + name, num_threads=default_num_threads)
        if allow_ensembling and not isfile(join(base, "postprocessing.json")):
            determine_postprocessing(base, gt_folder, "ensembled_raw", "temp", "ensembled_postprocessed", default_num_threads, dice_threshold=0)
            final = join(base, "ensembled_postprocessed", "summary.json")
            json_out = load_json(final)
            json_out["experiment_name"] = name
            save_json(json_out, final)
            os.makedirs(out_dir_all_json, exist_ok=True)
            shutil.copy(final, join(out_dir_all_json, "%s__%s.json" % (task, name)))


def ensemble(training_output_folder1, training_output_folder2, output_folder, task, validation_folder, folds, gt_folder,
             allow_ensembling=True, regions_class_order_from_pkl=False):
    """ensemble.py:39-123: the two-model ensemble of every validation case of every fold into output_folder/ensembled_raw (+ summary.json),
    then, with allow_ensembling, its postprocessing decision.  output_folder is OUT/ensembles/<task>/ensemble_<NAME1>--<NAME2>: the
    postprocessed summary is copied to OUT/summary_jsons.  gt_folder: the ground-truth label files (the reference's gt_segmentations)."""
    out = os.path.dirname(os.path.dirname(os.path.dirname(os.path.normpath(output_folder))))
    _ensemble_pairs([training_output_folder1, training_output_folder2], [(0, 1)], {(0, 1): output_folder}, task, validation_folder, folds,
                    gt_folder, allow_ensembling, regions_class_order_from_pkl, join(out, "summary_jsons"))


def _predict_line(n, folder, npz):
    return "python -m cineflow.predict -i FOLDER_WITH_TEST_CASES -o OUTPUT_FOLDER_MODEL%d -m %s%s\n" % (n, folder, " -z" if npz else "")


def find_best_configuration(models, gt_folder, output_folder, validation_folder="validation_raw", folds=(0, 1, 2, 3, 4), task="Task",
                            disable_ensembling=False, disable_postprocessing=False, regions_class_order_from_pkl=False):
    """figure_out_what_to_submit.py:94-238 for one task.  models: ordered {NAME: trainer output folder}.  Writes
    output_folder/prediction_commands.txt and summary.csv (and the ensembles under output_folder/ensembles/<task>/) and returns
    (best name, {name: mean foreground Dice})."""
    models = OrderedDict(models)
    folds = tuple(int(i) for i in folds)
    results, all_results, valid_models = OrderedDict(), OrderedDict(), []
    for m, folder in models.items():
        if not isdir(folder):
            raise RuntimeError("Output folder for model %s is missing, expected: %s" % (m, folder))
        cv_niftis_folder = join(folder, "cv_niftis_raw")
        if disable_postprocessing:
            if not isfile(join(cv_niftis_folder, "summary.json")):
                print(task, m, ": collecting niftis from 5-fold cv")
                if isdir(cv_niftis_folder):
                    shutil.rmtree(cv_niftis_folder)
                collect_cv_niftis(folder, cv_niftis_folder, validation_folder, folds)
                niftis_gt = subfiles(join(folder, "gt_niftis"), suffix=".nii.gz", join_=False)
                niftis_cv = subfiles(cv_niftis_folder, suffix=".nii.gz", join_=False)
                if not all(i in niftis_gt for i in niftis_cv):
                    raise AssertionError("It does not seem like you trained all the folds! Train "
                                         "all folds first! There are %d gt niftis in %s but only "
                                         "%d predicted niftis in %s" % (len(niftis_gt), niftis_gt, len(niftis_cv), niftis_cv))
                summary_fold0 = load_json(join(folder, "fold_%d" % folds[0], validation_folder, "summary.json"))["results"]["mean"]
                classes = tuple(int(i) for i in summary_fold0.keys())
                print(task, m, ": evaluating 5-fold cv results")
                evaluate_folder(join(folder, "gt_niftis"), cv_niftis_folder, classes)
        else:
            postprocessing_json = join(folder, "postprocessing.json")
            if not isfile(postprocessing_json) or not isdir(cv_niftis_folder):
                print("running missing postprocessing for %s and model %s" % (task, m))
                consolidate_folds(folder, folds=folds, validation_folder_name=validation_folder)
            assert isfile(postprocessing_json), "Postprocessing json missing, expected: %s" % postprocessing_json
            assert isdir(cv_niftis_folder), "Folder with niftis from CV missing, expected: %s" % cv_niftis_folder
        summary_file = join(cv_niftis_folder, "summary.json")
        results[m] = get_mean_foreground_dice(summary_file)
        foreground_mean(summary_file)
        all_results[m] = load_json(summary_file)["results"]["mean"]
        valid_models.append(m)

    ensembles_root = join(output_folder, "ensembles", task)
    if not disable_ensembling:
        print("\nI will now ensemble combinations of the following models:\n", valid_models)
        if len(valid_models) > 1:
            folders = [models[m] for m in valid_models]
            wanted = list(combinations(range(len(valid_models)), 2))
            names = {(a, b): ensemble_name(valid_models[a], valid_models[b]) for a, b in wanted}
            bases = {ab: join(ensembles_root, names[ab]) for ab in wanted}
            for ab in wanted:
                os.makedirs(bases[ab], exist_ok=True)
                print("ensembling", folders[ab[0]], folders[ab[1]])
            _ensemble_pairs(folders, wanted, bases, task, validation_folder, folds, gt_folder, not disable_postprocessing,
                            regions_class_order_from_pkl, join(output_folder, "summary_jsons"))
            for ab in wanted:
                summary_file = join(bases[ab], "ensembled_raw", "summary.json")
                results[names[ab]] = get_mean_foreground_dice(summary_file)
                foreground_mean(summary_file)
                all_results[names[ab]] = load_json(summary_file)["results"]["mean"]

    best = np.max(list(results.values()))
    for k, v in results.items():
        print(k, v)
    predict_str = ""
    best_model = None
    for k, v in results.items():
        if v == best:                                                # every entry equal to the maximum appends its commands; the last one is named
            print("%s submit model %s" % (task, k), v)
            best_model = k
            print("\nHere is how you should predict test cases. Run in sequential order and replace all input and output folder names with your "
                  "personalized ones\n")
            if k.startswith("ensemble"):
                model1, model2 = k[len("ensemble_"):].split("--")
                predict_str += _predict_line(1, models[model1], True)
                predict_str += _predict_line(2, models[model2], True)
                predict_str += "python -m cineflow.ensemble_predictions -f OUTPUT_FOLDER_MODEL1 OUTPUT_FOLDER_MODEL2 -o OUTPUT_FOLDER"
                if not disable_postprocessing:
                    predict_str += " -pp " + join(ensembles_root, k, "postprocessing.json")
                predict_str += "\n"
            else:
                predict_str += _predict_line(1, models[k], False)
            print(predict_str)

    os.makedirs(output_folder, exist_ok=True)
    with open(join(output_folder, "prediction_commands.txt"), "w") as f:
        f.write(predict_str)
    num_classes = len([i for i in all_results[best_model].keys() if i != "mean" and i != "0"])
    with open(join(output_folder, "summary.csv"), "w") as f:
        f.write("model")
        for c in range(1, num_classes + 1):
            f.write(",class%d" % c)
        f.write(",average")
        f.write("\n")
        for m in all_results.keys():
            f.write(m)
            for c in range(1, num_classes + 1):
                f.write(",%01.4f" % all_results[m][str(c)]["Dice"])
            f.write(",%01.4f" % all_results[m]["mean"]["Dice"])
            f.write("\n")
    return best_model, results


def parse_models(specs):
    """-m NAME=FOLDER ... -> ordered {NAME: FOLDER}; NAME is `<model>__<trainer>__<plans>` and must be unique"""
    models = OrderedDict()
    for spec in specs:
        name, sep, folder = spec.partition("=")
        if not sep or not name or not folder:
            raise ValueError("-m %r is not NAME=FOLDER" % (spec,))
        if len(name.split("__")) != 3 or "--" in name:
            raise ValueError("-m %r: NAME must be <model>__<trainer>__<plans> (it is split at '__' and joined with '--')" % (spec,))
        if name in models:
            raise ValueError("-m %r: the name is given twice" % (spec,))
        models[name] = folder
    return models


def build_parser():
    parser = argparse.ArgumentParser(description="Identify the best model, or pair of models, from the cross-validation of trained model folders: "
                                                 "scores every model and every two-model ensemble and writes the commands that predict the test set.")
    parser.add_argument("-m", "--models", nargs="+", required=True, metavar="NAME=FOLDER",
                        help="trainer output folders (plans.pkl, gt_niftis, fold_X/<val>/), named <model>__<trainer>__<plans>")
    parser.add_argument("-gt", required=True, type=str, help="folder of the ground-truth label files (.nii.gz) the ensembles are scored against")
    parser.add_argument("-o", "--output_folder", required=True, type=str, help="prediction_commands.txt, summary.csv and ensembles/ go here")
    parser.add_argument("-val", "--validation_folder", type=str, default="validation_raw", help="folder of a fold that holds its predictions")
    parser.add_argument("-f", "--folds", nargs="+", type=int, default=(0, 1, 2, 3, 4))
    parser.add_argument("-t", "--task_name", type=str, default="Task", help="task name, used in folder and summary names")
    parser.add_argument("--disable_ensembling", default=False, action="store_true", help="find the best single model only")
    parser.add_argument("--disable_postprocessing", default=False, action="store_true", help="do not determine or use postprocessing")
    parser.add_argument("--regions_class_order_from_pkl", default=False, action="store_true",
                        help="label region-based members by the regions_class_order of their .pkl (the reference takes the arg-max)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    best, _ = find_best_configuration(parse_models(args.models), args.gt, args.output_folder, args.validation_folder, args.folds,
                                      args.task_name, args.disable_ensembling, args.disable_postprocessing, args.regions_class_order_from_pkl)
    return best


if __name__ == "__main__":
    main()
