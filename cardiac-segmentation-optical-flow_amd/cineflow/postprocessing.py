"""Deciding which classes get the largest-connected-component filter, on the device: the interface and the rules of
nnunet/postprocessing/connected_components.py:123-447 (determine_postprocessing, apply_postprocessing_to_folder) and
consolidate_postprocessing.py:25-86 (collect_cv_niftis, consolidate_folds), restated.

The reference filters every validation case 2 (K + 1) + K times and writes three folders of temporary NIfTI files between the steps.  Here
a case is read once and judged in one visit: two cf_cc_label calls (all foreground as one object, every class on its own), cf_cc_sizes,
and one cf_pp_confusion that counts TP / FP / FN of the raw prediction and of its three filtered variants without writing an image.  The
host forms the per-case Dice of every variant from those integers with cineflow.metrics (same float64 expressions and NaN rules as
aggregate_scores), takes the np.nanmean over the cases and decides by the reference's rules.  Files are only written for the final
folder -- and, with debug=True (the reference's default), for temp_allClasses/ and temp_perClass/ -- by cf_cc_apply from the same
label maps.

Memory: every case of the folder stays on the device until the decisions are made (the prediction, the ground truth, two int32 label maps
and two int32 count arrays: 18 bytes per voxel, plus the host copies of the files).  A few hundred cardiac cases are a few GB; a folder of
several hundred CT-sized volumes does not fit and has to be split.

    python -m cineflow.postprocessing -f EXPERIMENT_FOLDER          # consolidate_folds
"""
import os
import shutil
import time
from concurrent.futures import ThreadPoolExecutor
from os.path import isdir, isfile, join

import numpy as np
import torch

from . import metrics, ops
from .evaluation import aggregate_scores
from .export import load_remove_save
from .folder_io import Loaded, load_json, load_volume, save_json, subfiles
from .metrics import ConfusionMatrix, label_volume_u8
from .nifti import write_nifti

default_num_threads = 1          # nnunet/configuration.py:4

# seconds of the last determine_postprocessing call: `read_s` is summed over the reader threads (reading + inflating), `wall_s` the whole call
LAST_TIMING = {}


def _timed_load(path):
    t0 = time.perf_counter()
    v = load_volume(path)
    LAST_TIMING["read_s"] = LAST_TIMING.get("read_s", 0.0) + time.perf_counter() - t0       # (float add under the GIL)
    return v


class _Case:
    """One file of the raw folder on the device with its two label maps (threshold-independent, made once)."""

    def __init__(self, pred, gt, classes, K, binary):
        self.pred_loaded, self.gt_loaded = pred, gt
        self.pred = label_volume_u8(pred.array, pred.path)
        self.volume_per_voxel = float(np.prod(pred.props["itk_spacing"], dtype=np.float64))
        self.gt = None
        if gt is not None:
            self.gt = label_volume_u8((gt.array > 0).astype(np.uint8) if binary else gt.array, gt.path)
            metrics.assert_shape(self.pred, self.gt)
        self.classes, self.K = classes, K
        self.fg_table, self.cls_table = {c: 1 for c in classes}, {c: c for c in classes}
        self.labels_fg = ops.connected_component_labels(self.pred, self.fg_table)
        self.labels_cls = ops.connected_component_labels(self.pred, self.cls_table)
        self.counts_fg, self.max_fg = ops.connected_component_sizes(self.labels_fg, self.pred, self.fg_table)
        self.counts_cls = self.max_cls = self.max_cls_alive = None

    def judge(self, min_valid):
        """The what-if pass with thresholds `min_valid` ({0: foreground, c: class c} in voxel-volume units, None: remove always) ->
        (counts int64 [4, K, 3] or None without a ground truth, largest foreground object, largest object per class in the raw image,
        largest object per class after the foreground step), sizes in voxels."""
        after_fg = ops.cc_apply(self.pred, self.K, True, [], self.labels_fg, self.counts_fg, self.max_fg, None, None, None, self.volume_per_voxel,
                                min_valid)
        self.counts_cls, self.max_cls, self.max_cls_alive = ops.connected_component_sizes(self.labels_cls, self.pred, self.cls_table, alive=after_fg)
        counts = None
        if self.gt is not None:
            counts = ops.pp_confusion(self.pred, self.gt, self.K, self.labels_fg, self.counts_fg, self.max_fg, self.labels_cls, self.counts_cls,
                                      self.max_cls, self.max_cls_alive, self.volume_per_voxel, min_valid).cpu().numpy()
        mx = torch.cat([self.max_fg[1:2], self.max_cls[:self.K], self.max_cls_alive[:self.K]]).cpu().numpy()
        return counts, int(mx[0]), mx[1:1 + self.K], mx[1 + self.K:]

    def filtered(self, do_fg, single_classes, min_valid):
        """the image after "foreground step yes/no + these single classes" (needs a judge() with the same foreground threshold before)"""
        return ops.cc_apply(self.pred, self.K, do_fg, single_classes, self.labels_fg, self.counts_fg, self.max_fg, self.labels_cls, self.counts_cls,
                            self.max_cls_alive if do_fg else self.max_cls, self.volume_per_voxel, min_valid)


def _dice(counts, c):
    """Dice of class c from {TP, FP, FN}, through cineflow.metrics.dice like every summary.json value"""
    cm = ConfusionMatrix()
    tp, fp, fn = (int(v) for v in counts[c])
    cm.tp, cm.fp, cm.fn, cm.tn = tp, fp, fn, 0
    cm.test_empty, cm.reference_empty, cm.test_full, cm.reference_full = tp + fp == 0, tp + fn == 0, False, False
    return metrics.dice(confusion_matrix=cm)


def _mean_dice(per_case_counts, variant, classes):
    """{str(c): float(np.nanmean(per-case Dice))} -- the 'mean' entry aggregate_scores would write for this variant"""
    return {str(c): float(np.nanmean([_dice(counts[variant], c) for counts in per_case_counts])) for c in classes}


def _kept(sizes_in_voxels, volumes):
    """min over the files of the largest object's size (load_remove_save's kept_size; files without an object do not count)"""
    vals = [float(s * v) for s, v in zip(sizes_in_voxels, volumes) if s > 0]
    return min(vals) if vals else None


def determine_postprocessing(base, gt_labels_folder, raw_subfolder_name="validation_raw", temp_folder="temp", final_subf_name="validation_final",
                             processes=default_num_threads, dice_threshold=0, debug=True, advanced_postprocessing=False,
                             pp_filename="postprocessing.json", log_function=print, metadata_list=None, binary=False, to_validate_list=None,
                             nb_threads=1):
    """Decides from the files of base/raw_subfolder_name (which must hold a summary.json) and the ground truth of gt_labels_folder whether
    keeping only the largest foreground object, and then only the largest object of single classes, raises the mean Dice; writes
    base/pp_filename and the filtered files plus their summary.json to base/final_subf_name.

    Rules (connected_components.py:253-388): the foreground step is taken when some class gains more than dice_threshold and none loses;
    after it (on its result when taken, else on the raw files) a class gets its own step when it gains more than dice_threshold.
    advanced_postprocessing: objects are only removed below the smallest "largest object" found in any file.  Evaluated files are those in
    to_validate_list, or without it those whose name has no '_u'.  debug: also write temp_folder + "_allClasses" / "_perClass" (otherwise no
    temporary file is written).  processes, nb_threads: reader / writer threads."""
    raw_folder, final_folder = join(base, raw_subfolder_name), join(base, final_subf_name)
    assert isfile(join(raw_folder, "summary.json")), "join(base, raw_subfolder_name) does not contain a summary.json"
    raw_results = load_json(join(raw_folder, "summary.json"))["results"]
    classes = [int(k) for k in raw_results["mean"] if int(k) != 0]
    K = max(classes) + 1
    if K > ops.PP_KMAX:
        raise ValueError("determine_postprocessing: class values up to %d; the device route holds labels below %d" % (K - 1, ops.PP_KMAX))
    dice_raw = {str(c): raw_results["mean"][str(c)]["Dice"] for c in classes}           # as scored by whoever wrote the raw summary
    key_fg = tuple(classes)

    step_folders = {"fg": join(base, temp_folder + "_allClasses"), "cls": join(base, temp_folder + "_perClass")}
    for folder in step_folders.values():
        shutil.rmtree(folder, ignore_errors=True)
        if debug:
            os.makedirs(folder)
    os.makedirs(final_folder, exist_ok=True)

    fnames = subfiles(raw_folder, suffix=".nii.gz", join_=False)
    evaluated = [(f in to_validate_list) if to_validate_list is not None else ("_u" not in f) for f in fnames]
    scored = [i for i, e in enumerate(evaluated) if e]

    LAST_TIMING.clear()
    t_start = time.perf_counter()
    pool = ThreadPoolExecutor(max(1, min(16, max(int(nb_threads or 1), int(processes or 1)))))
    try:
        # every file is read once: the prediction, and the ground truth of the files that are evaluated
        reads = [(pool.submit(_timed_load, join(raw_folder, f)), pool.submit(_timed_load, join(gt_labels_folder, f)) if e else None)
                 for f, e in zip(fnames, evaluated)]
        cases = [_Case(p.result(), g.result() if g is not None else None, classes, K, binary) for p, g in reads]
        volumes = [c.volume_per_voxel for c in cases]

        def judge_all(min_valid):
            res = [c.judge(min_valid) for c in cases]
            return [res[i][0] for i in scored], [r[1] for r in res], [r[2] for r in res], [r[3] for r in res]

        def write_folder(folder, do_fg, single_classes, min_valid):
            """the images of one step as files plus their summary.json (aggregate_scores on the volumes in memory)"""
            writes, pairs = [], []
            for i, (f, c) in enumerate(zip(fnames, cases)):
                img = c.filtered(do_fg, single_classes, min_valid).cpu().numpy().astype(c.pred_loaded.array.dtype)
                p = c.pred_loaded.props
                writes.append(pool.submit(write_nifti, join(folder, f), img, p["itk_spacing"], p["itk_origin"], p["itk_direction"]))
                if evaluated[i]:
                    pairs.append([Loaded(join(folder, f), img, p), c.gt_loaded])
            for w in writes:
                w.result()
            aggregate_scores(pairs, labels=classes, json_output_file=join(folder, "summary.json"), json_author="Fabian", num_threads=processes,
                             advanced=True, metadata_list=metadata_list, binary=binary, nb_threads=nb_threads)

        # ---- step 1: all foreground classes as one region
        min_valid, sizes_fg_step = None, None
        if advanced_postprocessing:
            _, largest_fg, _, _ = judge_all(None)
            sizes_fg_step = {key_fg: _kept(largest_fg, volumes)}
            if sizes_fg_step[key_fg] is None:
                raise KeyError(key_fg)                                                   # no file holds a foreground object (as in the reference)
            log_function("foreground vs background, smallest valid object size was:", sizes_fg_step[key_fg])
            min_valid = {0: sizes_fg_step[key_fg]}
        counts, _, largest_cls_raw, largest_cls_alive = judge_all(min_valid)
        if debug:
            write_folder(step_folders["fg"], True, [], min_valid)
        log_function("33%")
        dice_fg = _mean_dice(counts, 1, classes)
        gained = [dice_fg[str(c)] > dice_raw[str(c)] + dice_threshold for c in classes]
        lost = [dice_fg[str(c)] < dice_raw[str(c)] for c in classes]
        do_fg = any(gained) and not any(lost)
        log_function("Foreground vs background")
        log_function("before:", np.mean([dice_raw[str(c)] for c in classes]))
        log_function("after: ", np.mean([dice_fg[str(c)] for c in classes]))

        for_which_classes, sizes_out = [], {}
        if do_fg:
            for_which_classes.append(classes)
            sizes_out.update(sizes_fg_step or {})
            log_function("Removing all but the largest foreground region improved results!")

        # ---- step 2: every class on its own, after step 1 when it was taken
        dice_cls = {}
        if len(classes) > 1:
            sizes_cls_step = None
            if advanced_postprocessing:
                source = largest_cls_alive if do_fg else largest_cls_raw
                sizes_cls_step = {c: _kept([s[c] for s in source], volumes) for c in classes}
                sizes_cls_step = {c: v for c, v in sizes_cls_step.items() if v is not None}
                log_function("classes treated separately, smallest valid object sizes are")
                log_function(sizes_cls_step)
                # a class no file holds has no threshold; its entry stays "remove always", which meets no object
                min_valid = {**min_valid, **sizes_cls_step}
                counts, _, _, _ = judge_all(min_valid)
            if debug:
                write_folder(step_folders["cls"], do_fg, classes, min_valid)
            log_function("66%")
            before = dice_fg if do_fg else dice_raw
            dice_cls = _mean_dice(counts, 3 if do_fg else 2, classes)
            for c in classes:
                log_function(c)
                log_function("before:", before[str(c)])
                log_function("after: ", dice_cls[str(c)])
                if dice_cls[str(c)] > before[str(c)] + dice_threshold:
                    for_which_classes.append(int(c))
                    if sizes_cls_step is not None:
                        sizes_out[c] = sizes_cls_step[c]
                    log_function("Removing all but the largest region for class", c, "improved results!")
        else:
            log_function("Only one class present, no need to do each class separately as this is covered in fg vs bg")

        if not advanced_postprocessing:
            sizes_out = None
        log_function("for which classes:", for_which_classes)
        log_function("min_object_sizes", sizes_out)

        # ---- the final folder (the foreground threshold is the one of the last what-if pass, so the cases' per-class maxima still hold)
        final_min_valid = None if sizes_out is None else {(0 if k == key_fg else k): v for k, v in sizes_out.items()}
        write_folder(final_folder, do_fg, [c for c in for_which_classes if not isinstance(c, list)], final_min_valid)

        # the json's keys and value spellings are the reference's (connected_components.py:171-177, 406-437): export.load_postprocessing and
        # the reference's own loader read it
        save_json({"dc_per_class_raw": dice_raw, "dc_per_class_pp_all": dice_fg, "dc_per_class_pp_per_class": dice_cls,
                   "for_which_classes": for_which_classes, "min_valid_object_sizes": str(sizes_out), "num_samples": len(raw_results["all"]),
                   "validation_raw": raw_subfolder_name, "validation_final": final_subf_name}, join(base, pp_filename))
    finally:
        pool.shutdown()
    LAST_TIMING["wall_s"] = time.perf_counter() - t_start
    log_function("done")


def apply_postprocessing_to_folder(input_folder, output_folder, for_which_classes, min_valid_object_size=None, num_processes=8):
    """The filter of `for_which_classes` on every .nii.gz of input_folder -> output_folder.  Any for_which_classes, joint regions such as
    [(1, 2), 3] included: file by file through export.load_remove_save (num_processes is accepted and unused)."""
    os.makedirs(output_folder, exist_ok=True)
    for name in subfiles(input_folder, suffix=".nii.gz", join_=False):
        load_remove_save(join(input_folder, name), join(output_folder, name), for_which_classes, min_valid_object_size)


def collect_cv_niftis(cv_folder, output_folder, validation_folder_name="validation_raw", folds=(0, 1, 2, 3, 4)):
    """Copies the .nii.gz files of cv_folder/fold_<f>/validation_folder_name of every fold into output_folder; a missing fold is an error.
    Differs from the reference on purpose: it indexes its folder list by the fold VALUE, which fails for folds such as (1, 3); here every
    listed fold's folder is copied."""
    folders = {f: join(cv_folder, "fold_%d" % f, validation_folder_name) for f in folds}
    missing = [f for f, folder in folders.items() if not isdir(folder)]
    if missing:
        raise RuntimeError("some folds are missing. Please run the full 5-fold cross-validation. "
                           "The following folds seem to be missing: %s" % missing)
    os.makedirs(output_folder, exist_ok=True)
    for folder in folders.values():
        for path in subfiles(folder, suffix=".nii.gz"):
            shutil.copy(path, output_folder)


def consolidate_folds(output_folder_base, validation_folder_name="validation_raw", advanced_postprocessing=False, folds=(0, 1, 2, 3, 4)):
    """One post-processing decision for a whole cross-validation: gathers the folds' validation files into cv_niftis_raw/ (made afresh),
    scores them against gt_niftis/ (which must hold as many files), and runs determine_postprocessing on the lot -> postprocessing.json
    and cv_niftis_postprocessed/ in output_folder_base.  The class list is the one of fold_0's summary.json."""
    raw = join(output_folder_base, "cv_niftis_raw")
    gt = join(output_folder_base, "gt_niftis")
    shutil.rmtree(raw, ignore_errors=True)
    collect_cv_niftis(output_folder_base, raw, validation_folder_name, folds)
    names = subfiles(raw, suffix=".nii.gz", join_=False)
    if len(names) != len(subfiles(gt, suffix=".nii.gz")):
        raise AssertionError("If does not seem like you trained all the folds! Train all folds first!")
    classes = [int(k) for k in load_json(join(output_folder_base, "fold_0", validation_folder_name, "summary.json"))["results"]["mean"]]
    no_metadata = [{}] * len(names)
    aggregate_scores([(join(raw, n), join(gt, n)) for n in names], labels=classes, json_output_file=join(raw, "summary.json"),
                     num_threads=default_num_threads, advanced=True, metadata_list=no_metadata)
    determine_postprocessing(output_folder_base, gt, "cv_niftis_raw", final_subf_name="cv_niftis_postprocessed", processes=default_num_threads,
                             advanced_postprocessing=advanced_postprocessing, metadata_list=no_metadata)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="consolidate_folds: one postprocessing.json for all folds of an experiment")
    parser.add_argument("-f", type=str, required=True, help="experiment folder holding fold_0, fold_1, ... and gt_niftis")
    return parser


def main(argv=None):
    consolidate_folds(build_parser().parse_args(argv).f)


if __name__ == "__main__":
    main()
