"""Validation of trained folds on the HIP path: what `nnUNet_train ... -val --npz` leaves behind, written from the stage folders of
cineflow.plan_and_preprocess and a model folder cineflow.predict serves.

Mirrors `nnUNetTrainer.validate` (nnunet/training/network_training/nnUNetTrainer.py:733-874 under nnUNetTrainerV2.py:189-205),
`load_dataset` (dataset_loading.py), `do_split` (nnUNetTrainerV2.py:282-353) and, for the cascade, `predict_next_stage` /
`resample_and_save` (nnunet/training/cascade_stuff/predict_next_stage.py:31-87).  The reference reads its folders from global path
variables and from the trainer; here every path is an argument:

    python -m cineflow.validate -m MODEL_FOLDER --data STAGE_FOLDER -gt GT_FOLDER -o EXPERIMENT
           [-f 0 1 ... | all] [--splits FILE] [--plans PLANS_PKL] [--val validation_raw] [--no_softmax] [--disable_tta]
           [--step_size 0.5] [--overwrite 0|1] [--disable_postprocessing] [--debug]
           [--next_stage STAGE_FOLDER] [--prev_stage PRED_NEXT_STAGE_FOLDER] [-t TASK]

It writes what cineflow.postprocessing and cineflow.model_selection read: EXPERIMENT/fold_X/<val>/{<case>.nii.gz, <case>.npz, <case>.pkl,
summary.json, validation_args.json}, EXPERIMENT/fold_X/{postprocessing.json, <val>_postprocessed/}, EXPERIMENT/gt_niftis/ and
EXPERIMENT/plans.pkl.  Fold X is validated with the weights of MODEL_FOLDER/fold_X alone.

A case is exported in ONE device visit: the softmax of the sliding window stays on the device, is permuted by transpose_backward there,
and one `cineflow.ops.resample_argmax` launch resamples it to the size before preprocessing, takes the label, places it in the volume
before cropping, rounds the probabilities to the stored fp16 and counts the 16 x 16 confusion against the uploaded ground truth.
summary.json is aggregate_scores' document built from those counts (`evaluation.Counted`): no written file is read back.  With
--next_stage the same softmax goes through the kernel once more, at the next stage's size (the reference predicts the case twice).

Differences that are deliberate:
  * the fork replaced the tail of validate by determine_postprocessing_custom_with_metrics, which needs its dataset's metadata; this
    command writes stock nnU-Net's tail (aggregate_scores with labels range(num_classes), then determine_postprocessing), which is what
    the two consumers here read;
  * splits_final.pkl is made without scikit-learn (the seeded shuffle-and-cut of KFold in numpy, same folds) and read through the safe
    unpickler; an odd number of cases is refused with a ValueError (the fork's pairing fails an assertion);
  * a model folder with a flow network is refused: the flow trainers' validate_flow_* are not built."""
import argparse
import json
import os
import pickle
import shutil
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from os.path import isdir, isfile, join

import numpy as np

from .folder_io import load_volume, read_ahead, save_json, subfiles
from .safe_pickle import load_plain_pickle

default_num_threads = 8
MAX_IO_THREADS = 16
NEXT_STAGE_SUFFIX = "_segFromPrevStage.npz"


# ------------------------------------------------------------------------------------------------ dataset and split
def load_dataset(folder):
    """dataset_loading.py load_dataset: the cases of a stage folder, sorted -> ordered {case: {'data_file': <case>.npz,
    'properties_file': <case>.pkl}} (segFromPrevStage files are no cases)."""
    if not isdir(folder):
        raise FileNotFoundError("stage folder %s does not exist" % folder)
    ids = sorted(f[:-4] for f in subfiles(folder, suffix=".npz", join_=False) if "segFromPrevStage" not in f)
    return OrderedDict((c, OrderedDict([("data_file", join(folder, c + ".npz")), ("properties_file", join(folder, c + ".pkl"))])) for c in ids)


def kfold_indices(n, n_splits=5, seed=12345):
    """sklearn.model_selection.KFold(n_splits, shuffle=True, random_state=seed).split(range(n)) -> [(train_idx, test_idx)], both ascending:
    one seeded shuffle of range(n), cut into n_splits runs whose first n % n_splits are one longer."""
    if n < n_splits:
        raise ValueError("Cannot have number of splits n_splits=%d greater than the number of samples: n_samples=%d." % (n_splits, n))
    shuffled = np.arange(n)
    np.random.RandomState(seed).shuffle(shuffled)
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[:n % n_splits] += 1
    stops = np.cumsum(sizes)
    tests = [np.sort(shuffled[stop - size:stop]) for size, stop in zip(sizes, stops)]
    return [(np.setdiff1d(np.arange(n), t), t) for t in tests]


def create_splits(keys):
    """nnUNetTrainerV2.py:299-319: five folds over PAIRS of adjacent sorted keys (the two frames of a patient stay together)."""
    keys = np.sort(list(keys))
    if len(keys) % 2:
        raise ValueError("%d cases: the split pairs adjacent sorted cases (the two frames of a patient), so their number must be even"
                         % len(keys))
    splits = []
    for train_idx, test_idx in kfold_indices(len(keys) // 2):
        train_idx = np.sort(np.concatenate([train_idx * 2, train_idx * 2 + 1]))
        test_idx = np.sort(np.concatenate([test_idx * 2, test_idx * 2 + 1]))
        splits.append(OrderedDict([("train", keys[train_idx]), ("val", keys[test_idx])]))
    return splits


def do_split(keys, fold, splits_file):
    """nnUNetTrainerV2.py:282-353 -> (train keys, validation keys), both sorted lists.  fold 'all': every key on both sides.  splits_file
    is used when present and created (create_splits) when absent; a fold number beyond the file gives the seeded 80:20 split."""
    keys = sorted(str(k) for k in keys)
    if str(fold) == "all":
        return list(keys), list(keys)
    fold = int(fold)
    if not isfile(splits_file):
        print("Creating new 5-fold cross-validation split...")
        splits = create_splits(keys)
        with open(splits_file, "wb") as f:
            pickle.dump(splits, f)
    else:
        print("Using splits from existing split file:", splits_file)
        splits = load_plain_pickle(splits_file)
        print("The split file contains %d splits." % len(splits))
    if fold < len(splits):
        tr_keys, val_keys = [str(k) for k in splits[fold]["train"]], [str(k) for k in splits[fold]["val"]]
        unknown = [k for k in tr_keys + val_keys if k not in set(keys)]
        if unknown:
            raise KeyError("%s names cases the stage folder does not hold: %s" % (splits_file, unknown[:5]))
    else:
        print("INFO: You requested fold %d for training but splits contain only %d folds. I am now creating a random (but seeded) 80:20 split!"
              % (fold, len(splits)))
        rnd = np.random.RandomState(seed=12345 + fold)
        idx_tr = rnd.choice(len(keys), int(len(keys) * 0.8), replace=False)
        taken = set(int(i) for i in idx_tr)
        tr_keys, val_keys = [keys[i] for i in idx_tr], [keys[i] for i in range(len(keys)) if i not in taken]
    return sorted(tr_keys), sorted(val_keys)


# ------------------------------------------------------------------------------------------------ model folder
def check_model_folder(model_folder):
    """the plans.json of a segmentation-only model folder; one with a flow network is refused before anything is loaded"""
    plans_file = join(model_folder, "plans.json")
    if not isfile(plans_file):
        raise FileNotFoundError("Folder with saved model weights must contain a plans.json file (%s)" % model_folder)
    with open(plans_file) as f:
        plans = json.load(f)
    if plans.get("flow_net"):
        raise ValueError("%s holds 'flow_net': cineflow.validate validates segmentation-only model folders (the flow trainers' "
                         "validate_flow_* are not built)" % plans_file)
    return plans


def _export_params(plans, segmentation_export_kwargs):
    """nnUNetTrainer.py:752-764 -> (force_separate_z, interpolation_order, interpolation_order_z)"""
    kw = segmentation_export_kwargs if segmentation_export_kwargs is not None else plans.get("segmentation_export_params")
    if kw is None:
        return None, 1, 0
    return kw["force_separate_z"], kw["interpolation_order"], kw["interpolation_order_z"]


def _check_orders(order, order_z):
    if order not in (0, 1) or order_z not in (0, 1):
        raise NotImplementedError("export resampling is built for interpolation orders 0 and 1 (got %s / %s)" % (order, order_z))


def linear_flags(properties, force_separate_z, order, order_z):
    """The separate-z decision of save_segmentation_nifti_from_softmax (cineflow/export.py, segmentation_export.py:88-98) as the per-axis
    `linear` flags of ops.resize3d / ops.resample_argmax, in the axis order of the files."""
    from .export import get_do_separate_z, get_lowres_axis
    _check_orders(order, order_z)
    if force_separate_z is None:
        if get_do_separate_z(properties.get("original_spacing")):
            do_separate_z, lowres_axis = True, get_lowres_axis(properties.get("original_spacing"))
        elif get_do_separate_z(properties.get("spacing_after_resampling")):
            do_separate_z, lowres_axis = True, get_lowres_axis(properties.get("spacing_after_resampling"))
        else:
            do_separate_z, lowres_axis = False, None
    else:
        do_separate_z = force_separate_z
        lowres_axis = get_lowres_axis(properties.get("original_spacing")) if do_separate_z else None
    if lowres_axis is not None and len(lowres_axis) != 1:
        do_separate_z = False
    lin = [int(order)] * 3
    if do_separate_z:
        lin[int(lowres_axis[0])] = int(order_z)
    return tuple(lin)


def _placement(properties):
    """(size after cropping, size before cropping, origin of the crop) of a case, as the exporter places it"""
    crop = tuple(int(v) for v in properties["size_after_cropping"])
    bbox = properties.get("crop_bbox")
    if bbox is None:
        return crop, crop, (0, 0, 0)
    return crop, tuple(int(v) for v in properties["original_size_of_raw_data"]), tuple(int(b[0]) for b in bbox)


# ------------------------------------------------------------------------------------------------ one case
def case_name(properties):
    """nnUNetTrainer.py:804: the name of the case's label file"""
    return os.path.basename(properties["list_of_data_files"][0])[:-12]


def _read_case(job):
    """what one validation case needs from the disk, read on a pool thread: (data without the label channel, properties, ground truth or
    None, previous-stage labels or None, next-stage shape or None)"""
    case, entry, gt_file, prev_file, next_file = job
    data = np.load(entry["data_file"])["data"][:-1]
    properties = load_plain_pickle(entry["properties_file"])
    gt = load_volume(gt_file).array if gt_file is not None else None
    prev = None
    if prev_file is not None:
        if not isfile(prev_file):
            raise FileNotFoundError("case %s: the previous stage's labels %s are missing" % (case, prev_file))
        prev = np.load(prev_file)["data"]
    nxt = None
    if next_file is not None:
        if not isfile(next_file):
            raise FileNotFoundError("case %s: the next stage's file %s is missing" % (case, next_file))
        nxt = tuple(int(v) for v in np.load(next_file)["data"].shape[1:])
    return data, properties, gt, prev, nxt


def _with_prev_stage(trainer, data, prev, case):
    """nnUNetTrainerV2_CascadeFullRes.py:190ff: the previous stage's labels, one-hot over prev_stage_classes, behind the modalities"""
    import torch
    from . import ops
    prev = np.asarray(prev)
    if prev.ndim == 4 and prev.shape[0] == 1:
        prev = prev[0]
    if prev.ndim != 3:
        raise ValueError("case %s: previous-stage labels of shape %s (a [X,Y,Z] volume is expected)" % (case, prev.shape))
    dev = torch.device("cuda", torch.cuda.current_device())
    onehot = torch.empty((len(trainer.prev_stage_classes),) + tuple(data.shape[1:]), dtype=torch.float32, device=dev)
    ops.prev_stage_onehot(torch.from_numpy(np.ascontiguousarray(prev.astype(np.uint8))).to(dev), trainer.prev_stage_classes, onehot)
    return np.concatenate([np.asarray(data, dtype=np.float32), onehot.cpu().numpy()], axis=0)


def export_case(softmax, properties, transpose_backward, force_separate_z, order, order_z, regions_class_order, want_probs, gt, on_device=False):
    """The one-visit export: softmax, a device tensor [K, *stage shape] in the network's axis order -> (labels uint8 numpy at the size before
    cropping, stored fp16 probabilities numpy [K, *size_after_cropping] or None, hist int64 numpy [257] or None).  gt: the case's ground
    truth (numpy, the size before cropping) or None."""
    from . import ops
    from .metrics import label_volume_u8
    tb = [int(i) for i in transpose_backward]
    if tb != [0, 1, 2]:
        softmax = softmax.permute([0] + [i + 1 for i in tb])
    softmax = softmax.contiguous()
    crop, full, lo = _placement(properties)
    lin = linear_flags(properties, force_separate_z, order, order_z) if tuple(softmax.shape[1:]) != crop else (int(order),) * 3
    gt_t = None
    if gt is not None:
        if tuple(gt.shape) != full:
            raise ValueError("%s: the ground truth is %s, the case's original size is %s" % (case_name(properties), tuple(gt.shape), full))
        gt_t = label_volume_u8(gt, case_name(properties))
    seg, probs, hist = ops.resample_argmax(softmax, crop, lin, full_shape=full, bbox_lo=lo, regions_class_order=regions_class_order,
                                           want_probs=want_probs, gt=gt_t)
    if on_device:               # (compress="device": labels and probabilities stay where they are compressed)
        return seg, probs, None if hist is None else hist.cpu().numpy()
    return seg.cpu().numpy(), None if probs is None else probs.cpu().numpy(), None if hist is None else hist.cpu().numpy()


def _pack_case(out_file, seg, probs, properties):
    """compress="device", in the device loop: device labels and probabilities -> (the .nii.gz file's bytes, the softmax's deflate.Member or
    None); the raw arrays are not read back"""
    from . import deflate
    from .nifti import nifti_device_bytes
    return (nifti_device_bytes(out_file, seg, properties["itk_spacing"], properties["itk_origin"], properties["itk_direction"]),
            None if probs is None else deflate.npy_member(probs))


def _write_case(out_file, seg, probs, properties, regions_class_order, compress="zlib"):
    """the files save_segmentation_nifti_from_softmax(..., resampled_npz_fname=<case>.npz, properties_pkl=True) writes.  compress="device":
    seg and probs are what _pack_case made of them (finished bytes), or arrays that are packed now."""
    from .nifti import write_nifti
    if compress != "zlib":
        from . import deflate
        deflate.check_compress(compress)
        if not isinstance(seg, bytes):
            seg, probs = _pack_case(out_file, seg, probs, properties)
        if probs is not None:
            deflate.write_npz(out_file[:-7] + ".npz", {"softmax": probs})
            if regions_class_order is not None:
                properties["regions_class_order"] = regions_class_order
            with open(out_file[:-7] + ".pkl", "wb") as f:
                pickle.dump(properties, f)
        with open(out_file, "wb") as f:
            f.write(seg)
        return
    if probs is not None:
        np.savez_compressed(out_file[:-7] + ".npz", softmax=probs)
        if regions_class_order is not None:
            properties["regions_class_order"] = regions_class_order
        with open(out_file[:-7] + ".pkl", "wb") as f:
            pickle.dump(properties, f)
    write_nifti(out_file, seg, properties["itk_spacing"], properties["itk_origin"], properties["itk_direction"])


def resample_and_save(predicted, target_shape, output_file, force_separate_z=False, interpolation_order=1, interpolation_order_z=0,
                      compress="zlib"):
    """predict_next_stage.py:31-43: predicted, the device softmax [K,X,Y,Z] of the lower stage, at the next stage's shape as uint8 labels
    in `output_file` (`data=`); resampling and arg-max are one ops.resample_argmax launch.  compress="device": the labels are deflated
    where they are and returned as a device tensor."""
    import torch
    from . import ops
    _check_orders(interpolation_order, interpolation_order_z)
    if force_separate_z:
        raise ValueError("predict_next_stage: force_separate_z needs an anisotropic axis, which the stage folders do not name")
    if not torch.is_tensor(predicted):
        predicted = torch.from_numpy(np.ascontiguousarray(predicted, dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    seg = ops.resample_argmax(predicted.contiguous(), target_shape, (int(interpolation_order),) * 3)[0]
    if compress != "zlib":
        from . import deflate
        deflate.check_compress(compress)
        deflate.savez_compressed(output_file, data=seg)
        return seg
    seg = seg.cpu().numpy()
    np.savez_compressed(output_file, data=seg)
    return seg


# ------------------------------------------------------------------------------------------------ one fold
def _copy_shared(dataset, gt_folder, output_folder_base, plans_pkl):
    """EXPERIMENT/gt_niftis (the ground truth of every case of the stage folder) and EXPERIMENT/plans.pkl, each written once"""
    gt_out = join(output_folder_base, "gt_niftis")
    os.makedirs(gt_out, exist_ok=True)
    for entry in dataset.values():
        name = case_name(load_plain_pickle(entry["properties_file"])) + ".nii.gz"
        if not isfile(join(gt_out, name)):
            if not isfile(join(gt_folder, name)):
                raise FileNotFoundError("ground truth %s is missing" % join(gt_folder, name))
            shutil.copy(join(gt_folder, name), join(gt_out, name))
    if plans_pkl is not None and not isfile(join(output_folder_base, "plans.pkl")):
        shutil.copy(plans_pkl, join(output_folder_base, "plans.pkl"))
    return gt_out


def validate(trainer, params, fold, data_folder, gt_folder, output_folder_base, do_mirroring=True, use_sliding_window=True, step_size=0.5,
             save_softmax=True, use_gaussian=True, overwrite=True, validation_folder_name="validation_raw", debug=False,
             segmentation_export_kwargs=None, run_postprocessing_on_folds=True, splits_file=None, plans_pkl=None, task=None,
             next_stage_folder=None, prev_stage_folder=None, num_threads=default_num_threads, compress="zlib"):
    """nnUNetTrainer.validate for one fold: trainer / params as load_model_and_checkpoint_files(MODEL_FOLDER, [fold]) gives them (params: that
    fold's checkpoint dict).  Writes output_folder_base/fold_<fold>/<validation_folder_name>/ and what goes with it (module docstring) and
    returns that folder.  next_stage_folder: also predict_next_stage into output_folder_base/pred_next_stage; prev_stage_folder: where a
    cascade model finds <case>_segFromPrevStage.npz.  compress="device": validation_raw's .nii.gz / .npz and pred_next_stage's .npz are
    deflated and checksummed on the device in the case loop (cineflow.deflate); the writer threads get finished bytes."""
    import torch
    from .deflate import check_compress
    from .evaluation import Counted, HIST_K, aggregate_scores, evaluate_regions
    check_compress(compress)
    from .postprocessing import determine_postprocessing
    if trainer.flow_net is not None:
        raise ValueError("the model folder holds 'flow_net': cineflow.validate validates segmentation-only model folders")
    trainer.check_prev_stage(prev_stage_folder is not None)
    trainer.load_checkpoint_ram(params, False)
    plans = trainer.plans
    force_separate_z, order, order_z = _export_params(plans, segmentation_export_kwargs)
    _check_orders(order, order_z)
    regions_class_order = trainer.regions_class_order
    mirror_axes = trainer.data_aug_params["mirror_axes"] if do_mirroring else ()
    tb = list(plans.get("transpose_backward") or (0, 1, 2))

    dataset = load_dataset(data_folder)
    splits_file = splits_file or join(os.path.dirname(os.path.normpath(data_folder)), "splits_final.pkl")
    _tr_keys, val_keys = do_split(dataset.keys(), fold, splits_file)
    fold_folder = join(output_folder_base, "all" if str(fold) == "all" else "fold_%d" % int(fold))      # (nnUNetTrainer.py:292-298)
    output_folder = join(fold_folder, validation_folder_name)
    os.makedirs(output_folder, exist_ok=True)
    save_json({"do_mirroring": do_mirroring, "use_sliding_window": use_sliding_window, "step_size": step_size, "save_softmax": save_softmax,
               "use_gaussian": use_gaussian, "overwrite": overwrite, "validation_folder_name": validation_folder_name, "debug": debug,
               "all_in_gpu": False, "segmentation_export_kwargs": segmentation_export_kwargs}, join(output_folder, "validation_args.json"))
    gt_niftis = _copy_shared(dataset, gt_folder, output_folder_base, plans_pkl)
    next_out = None
    if next_stage_folder is not None:
        next_out = join(output_folder_base, "pred_next_stage")
        os.makedirs(next_out, exist_ok=True)

    threads = max(1, min(MAX_IO_THREADS, int(num_threads)))
    # a case whose files are all there is not predicted again without `overwrite`; its properties still name its label file
    jobs = []
    for case in val_keys:
        props = load_plain_pickle(dataset[case]["properties_file"])
        name = case_name(props)
        done = not overwrite and isfile(join(output_folder, name + ".nii.gz")) and (not save_softmax or isfile(join(output_folder, name + ".npz"))) \
            and (next_out is None or isfile(join(next_out, case + NEXT_STAGE_SUFFIX)))
        jobs.append((case, name, done))
    todo = [(case, dataset[case], join(gt_folder, name + ".nii.gz"),
             None if prev_stage_folder is None else join(prev_stage_folder, case + NEXT_STAGE_SUFFIX),
             None if next_stage_folder is None else join(next_stage_folder, case + ".npz")) for case, name, done in jobs if not done]
    in_histogram = trainer.num_classes <= HIST_K and all(0 <= int(c) < HIST_K for c in (regions_class_order or ()))
    counted = {}
    writers = ThreadPoolExecutor(threads)
    written = []
    try:
        for (job,), (loaded,) in read_ahead([(j,) for j in todo], _read_case, depth=threads, readers=threads):
            case = job[0]
            data, properties, gt, prev, next_shape = loaded
            name = case_name(properties)
            print(case, data.shape)
            if prev is not None:
                data = _with_prev_stage(trainer, data, prev, case)
            softmax = trainer.predict_preprocessed_data_return_seg_and_softmax(
                data, do_mirroring=do_mirroring, mirror_axes=mirror_axes, use_sliding_window=use_sliding_window, step_size=step_size,
                use_gaussian=use_gaussian, verbose=False, mixed_precision=trainer.mixed_precision, return_device=True)[1]
            seg, probs, hist = export_case(softmax, properties, tb, force_separate_z, order, order_z, regions_class_order, save_softmax, gt,
                                           on_device=compress != "zlib")
            out_file = join(output_folder, name + ".nii.gz")
            n_voxels = int(seg.numel() if torch.is_tensor(seg) else seg.size)
            if compress != "zlib":
                seg, probs = _pack_case(out_file, seg, probs, properties)
            written.append(writers.submit(_write_case, out_file, seg, probs, properties, regions_class_order, compress))
            if in_histogram and not hist[-1]:                           # every voxel of both volumes is below 16
                counted[name] = Counted(out_file, hist[:-1].reshape(HIST_K, HIST_K), n_voxels)
            if next_out is not None:
                resample_and_save(softmax, next_shape, join(next_out, case + NEXT_STAGE_SUFFIX), force_separate_z, order, order_z, compress)
            del softmax
        for w in written:
            w.result()
    finally:
        writers.shutdown(wait=True, cancel_futures=True)
    torch.cuda.synchronize()
    print("finished prediction")

    # the stock tail of validate: a case exported by this run brings its counts, one that was already there is scored from its file
    pairs = [(counted.get(name, join(output_folder, name + ".nii.gz")), join(gt_niftis, name + ".nii.gz")) for _case, name, _done in jobs]
    experiment = os.path.basename(os.path.normpath(output_folder_base))
    aggregate_scores(pairs, labels=list(range(trainer.num_classes)), json_output_file=join(output_folder, "summary.json"),
                     json_name=experiment + " val tiled %s" % str(use_sliding_window), json_author="Fabian",
                     json_task=task if task is not None else os.path.basename(os.path.dirname(os.path.normpath(data_folder))),
                     num_threads=default_num_threads)
    if run_postprocessing_on_folds:
        determine_postprocessing(fold_folder, gt_niftis, validation_folder_name, final_subf_name=validation_folder_name + "_postprocessed",
                                 debug=debug)
    if trainer.regions is not None:                                     # nnUNetTrainerV2BraTSRegions.validate
        evaluate_regions(output_folder, gt_niftis, OrderedDict((k, tuple(v)) for k, v in trainer.regions.items()))
    return output_folder


def predict_next_stage(trainer, params, fold, data_folder, stage_to_be_predicted_folder, output_folder_base, splits_file=None,
                       do_mirroring=True, step_size=0.5, num_threads=default_num_threads, compress="zlib"):
    """predict_next_stage.py:46-87 on its own: the validation cases of `fold` predicted by the lower stage and written at the next stage's
    shape to output_folder_base/pred_next_stage/<case>_segFromPrevStage.npz.  (validate(..., next_stage_folder=...) writes the same files
    from the softmax it already holds.)  Returns the folder."""
    trainer.load_checkpoint_ram(params, False)
    force_separate_z, order, order_z = _export_params(trainer.plans, None)
    dataset = load_dataset(data_folder)
    splits_file = splits_file or join(os.path.dirname(os.path.normpath(data_folder)), "splits_final.pkl")
    val_keys = do_split(dataset.keys(), fold, splits_file)[1]
    out = join(output_folder_base, "pred_next_stage")
    os.makedirs(out, exist_ok=True)
    threads = max(1, min(MAX_IO_THREADS, int(num_threads)))
    todo = [(case, dataset[case], None, None, join(stage_to_be_predicted_folder, case + ".npz")) for case in val_keys]
    for (job,), (loaded,) in read_ahead([(j,) for j in todo], _read_case, depth=threads, readers=threads):
        data, _properties, _gt, _prev, next_shape = loaded
        print(job[0])
        softmax = trainer.predict_preprocessed_data_return_seg_and_softmax(
            data, do_mirroring=do_mirroring, mirror_axes=trainer.data_aug_params["mirror_axes"] if do_mirroring else (), step_size=step_size,
            verbose=False, mixed_precision=trainer.mixed_precision, return_device=True)[1]
        resample_and_save(softmax, next_shape, join(out, job[0] + NEXT_STAGE_SUFFIX), force_separate_z, order, order_z, compress)
    return out


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    parser = argparse.ArgumentParser(description="validate trained folds: fold_X/validation_raw, gt_niftis and pred_next_stage of an experiment folder")
    parser.add_argument("-m", "--model_folder", required=True, help="segmentation-only model folder (plans.json, fold_X/<chk>.model)")
    parser.add_argument("--data", required=True, help="stage folder of the preprocessed task (<case>.npz / <case>.pkl)")
    parser.add_argument("-gt", "--gt_folder", required=True, help="ground-truth label files <case>.nii.gz (the task's labelsTr)")
    parser.add_argument("-o", "--output_folder", required=True, help="EXPERIMENT: the trainer output folder to write")
    parser.add_argument("-f", "--folds", nargs="+", default=None, help="fold numbers, or all (default: every fold_X of the model folder)")
    parser.add_argument("--splits", default=None, help="splits_final.pkl (default: next to the stage folder; created when absent)")
    parser.add_argument("--plans", default=None, help="plans.pkl of the task, copied to EXPERIMENT/plans.pkl")
    parser.add_argument("--val", default="validation_raw", help="name of the validation folder")
    parser.add_argument("--no_softmax", action="store_true", help="write no .npz / .pkl (nnUNet_train -val without --npz)")
    parser.add_argument("--disable_tta", action="store_true")
    parser.add_argument("--step_size", type=float, default=0.5)
    parser.add_argument("--overwrite", type=int, default=1)
    parser.add_argument("--disable_postprocessing", action="store_true")
    parser.add_argument("--debug", action="store_true", help="keep determine_postprocessing's temporary folders")
    parser.add_argument("--next_stage", default=None, help="the next stage's folder: also write EXPERIMENT/pred_next_stage (a 3d_lowres model)")
    parser.add_argument("--prev_stage", default=None, help="folder with <case>_segFromPrevStage.npz (a cascade model)")
    parser.add_argument("-t", "--task", default=None, help="task name of summary.json (default: the preprocessed task folder's name)")
    parser.add_argument("-chk", default="model_final_checkpoint")
    parser.add_argument("--compress", choices=("zlib", "device"), default="zlib", help="who deflates the .nii.gz / .npz files: zlib on the writer "
                        "threads (default) or the device, which hands back compressed bytes only; the contents are identical")
    return parser


def parse_folds(folds, model_folder):
    """-f: ints or 'all'; without it every fold_X of the model folder"""
    if folds is None:
        found = sorted(d[5:] for d in os.listdir(model_folder) if d.startswith("fold_") and isdir(join(model_folder, d)))
        if not found:
            raise FileNotFoundError("%s holds no fold_X folder" % model_folder)
        folds = found
    return [f if str(f) == "all" else int(f) for f in folds]


def main(argv=None):
    a = build_parser().parse_args(argv)
    check_model_folder(a.model_folder)
    folds = parse_folds(a.folds, a.model_folder)
    from .trainer import load_model_and_checkpoint_files
    out = []
    for fold in folds:
        trainer, params = load_model_and_checkpoint_files(a.model_folder, [fold], checkpoint_name=a.chk)
        out.append(validate(trainer, params[0], fold, a.data, a.gt_folder, a.output_folder, do_mirroring=not a.disable_tta, step_size=a.step_size,
                            save_softmax=not a.no_softmax, overwrite=bool(a.overwrite), validation_folder_name=a.val, debug=a.debug,
                            run_postprocessing_on_folds=not a.disable_postprocessing, splits_file=a.splits, plans_pkl=a.plans, task=a.task,
                            next_stage_folder=a.next_stage, prev_stage_folder=a.prev_stage, compress=a.compress))
    return out


if __name__ == "__main__":
    main()
