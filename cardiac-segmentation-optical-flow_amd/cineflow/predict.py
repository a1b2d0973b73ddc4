"""Predict-from-folder API of the reference, on the HIP path.

Mirrors `nnunet/inference/predict.py` (public names, argument lists and defaults of `predict_from_folder` :665-672,
`predict_cases` :228-232, `check_input_folder_and_return_caseIDs` :629, the CLI flags of :782-858) and the output
layout the downstream scripts read (`<out>/<patient>/{Segmentation,Registered}/<case>.nii.gz` uint8 and
`<out>/<patient>/Flow/<case>.npz` with `flow` float32 `[Y,X,Z,2]` + `spacing`, segmentation_export.py:190-219).

Differences that are deliberate and documented in DESIGN.md (those of the model folder and of the fold ensemble: cineflow.trainer):
  * every patient folder is processed (the reference `return`s from inside its patient loop, predict.py:743);
  * preprocessing is the reference's test-time chain driven by the plan entries (crop to non-zero, resampling to the
    stage spacing, the plans' normalisation schemes: `CineTrainer.preprocess_patient`, cineflow.preprocessing) and the
    exporter resamples back; the heart centroid of `Processor` comes from the cropping network of plans['cropping_net']
    when the folder has one (the reference's MTLmodel cropper), else from the patch centre;
  * when no ED label map is supplied the ED segmentation predicted by the U-Net is the one propagated;
  * a `plans.json` without 'flow_net' is a segmentation-only model (a plain 2-D nnU-Net folder): the dispatch of predict.py:320-353 then
    takes the predict_non_flow side -- every frame is written to `<out>/<patient>/<case>.nii.gz` (+ `<case>.npz` / `.pkl` with save_npz,
    :993-997), nothing under Flow/ or Registered/, postprocessing.json applied to those files; all frames of all patients of a device batch
    go through the cine-batched sliding window (cineflow.inference.predict_cine_2Dconv_tiled) in one call;
  * `predict_from_folder` loads the model once and fills the device batch ACROSS patients: the cropped slices of as many patients as fit
    `MAX_SLICES_PER_LAUNCH` (64) go through the networks as one batch (`CineTrainer.predict_patients_flow`), the next group's files are
    read and preprocessed by the `num_threads_preprocessing` pool meanwhile, and the NIfTI / NPZ export of finished patients runs in the
    `num_threads_nifti_save` pool while the device works on the next group.  The reference predicts and exports patient by patient
    (predict.py:228-354, :1008-1110); per-patient results are those of the one-patient call up to the launch shapes the batch size
    selects (tests/test_predict_api.py asserts the bound).  `LAST_TIMING` holds the wall-time split of the last call.
"""
import argparse
import csv
import itertools
import json
import os
import shutil
import sys
import threading
import time
from collections import deque
from copy import deepcopy
from multiprocessing.pool import ThreadPool

import numpy as np
import torch

from .export import load_postprocessing, load_remove_save, save_segmentation_nifti_from_softmax, subfiles
from .trainer import (API_PROFILE, DEVICE_SPLIT, CineTrainer, ModelWrapFlow, _cached_model, _check_prev_stage,  # noqa: F401  (re-exported: this module's API)
                      clear_model_cache, default_plans, load_model_and_checkpoint_files, save_model_folder)
from .voxelmorph_saver import write_raw

join = os.path.join

MAX_SLICES_PER_LAUNCH = int(os.environ.get("CF_API_SLICES", "64"))   # cropped cine slices per device batch of the file-level API
FIRST_BATCH_SLICES = int(os.environ.get("CF_API_FIRST_SLICES", "16"))     # slices of the first device batch of a predict_cases / predict_from_folder call
GIL_SWITCH_INTERVAL = float(os.environ.get("CF_API_SWITCH_INTERVAL", "0.0002"))   # seconds; Python's default is 0.005
_STREAM_POOL = {}                                                    # (device index) -> [torch.cuda.Stream]: reused by the preprocessing threads of every call
_STREAM_POOL_LOCK = threading.Lock()
LAST_TIMING = {}                                                     # wall-time split of the last predict_from_folder / predict_cases call


def _pooled_stream(device, k):
    with _STREAM_POOL_LOCK:
        pool = _STREAM_POOL.setdefault(torch.device(device).index or 0, [])
        while len(pool) <= k:
            pool.append(torch.cuda.Stream(device=device))
        return pool[k]


# ------------------------------------------------------------------------------------------------ predict API
def check_input_folder_and_return_caseIDs(input_folder, expected_num_modalities):
    """predict.py:629-662, message for message."""
    print("This model expects %d input modalities for each image" % expected_num_modalities)
    files = subfiles(input_folder, suffix=".nii.gz", join_=False, sort=True)
    maybe_case_ids = np.unique([i[:-12] for i in files])
    remaining = deepcopy(files)
    missing = []
    assert len(files) > 0, "input folder did not contain any images (expected to find .nii.gz file endings)"
    for c in maybe_case_ids:
        for n in range(expected_num_modalities):
            expected_output_file = c + "_%04.0d.nii.gz" % n
            if not os.path.isfile(join(input_folder, expected_output_file)):
                missing.append(expected_output_file)
            else:
                remaining.remove(expected_output_file)
    print("Found %d unique case ids, here are some examples:" % len(maybe_case_ids),
          np.random.choice(maybe_case_ids, min(len(maybe_case_ids), 10)))
    print("If they don't look right, make sure to double check your filenames. They must end with _0000.nii.gz etc")
    if len(remaining) > 0:
        print("found %d unexpected remaining files in the folder. Here are some examples:" % len(remaining),
              np.random.choice(remaining, min(len(remaining), 10)))
    if len(missing) > 0:
        print("Some files are missing:")
        print(missing)
        raise RuntimeError("missing files in input_folder")
    return maybe_case_ids


def _subfolder_path(path, sub):
    """predict.py:1059-1068 inserts the sub-folder as path component 2 of a relative path; this is the same place for
    `<out>/<patient>/<case>` and also works for absolute / nested output folders."""
    return join(os.path.dirname(path), sub, os.path.basename(path))


def get_ed_es_indices(csv_filepath):
    """predict.py:1196-1198: first row of the patient's csv, columns `ed_index`, `es_index`."""
    with open(csv_filepath) as f:
        rows = list(csv.DictReader(f))
    return int(float(rows[0]["ed_index"])), int(float(rows[0]["es_index"]))


def put_ed_first(current_list_of_lists, current_output_files, csv_filepath):
    """predict.py:1165-1193: rotate the frame list so that the end-diastolic frame comes first."""
    ed_index, _es = get_ed_es_indices(csv_filepath)
    order = list(range(ed_index, len(current_list_of_lists))) + list(range(0, ed_index))
    return [list(current_list_of_lists[i]) for i in order], [current_output_files[i] for i in order]


_VOXELMORPH_RAW = None


def set_voxelmorph_raw(pred_path, pkl_path=None):
    """Switch on (pred_path given) or off (None) the additional `<pred_path>/Raw/{Registered,Segmentation,Flow}/<patient>/` +
    `<pkl_path>/<case>.pkl` output of predict_flow -- the crop-space layout voxelmorph_saver_* post-processes.  A module-level switch, so
    that predict_from_folder / predict_cases keep the reference's argument lists; pkl_path defaults to <pred_path>/pkl."""
    global _VOXELMORPH_RAW
    _VOXELMORPH_RAW = None if pred_path is None else (pred_path, pkl_path or join(pred_path, "pkl"))


def _flow_outputs(out_fname):
    """the (Segmentation, Flow, Registered) files of the frame whose name is `<out>/<patient>/<case>.nii.gz`"""
    return _subfolder_path(out_fname, "Segmentation"), _subfolder_path(out_fname, "Flow")[:-7] + ".npz", _subfolder_path(out_fname, "Registered")


def _patient_folder(output_filenames):
    return os.path.abspath(os.path.dirname(output_filenames[0]))


def _export_kwargs(trainer, segmentation_export_kwargs):
    """predict.py:286-296: the caller's resampling settings, else the plans', as arguments of save_segmentation_nifti_from_softmax"""
    if segmentation_export_kwargs is None:
        exp = trainer.plans.get("segmentation_export_params") or {}
        return {"force_separate_z": exp.get("force_separate_z"), "order": exp.get("interpolation_order", 1),
                "interpolation_order_z": exp.get("interpolation_order_z", 0)}
    return {"force_separate_z": segmentation_export_kwargs["force_separate_z"], "order": segmentation_export_kwargs["interpolation_order"],
            "interpolation_order_z": segmentation_export_kwargs["interpolation_order_z"]}


def _to_file_axes(arr, plans):
    """back to the axis order of the files (predict.py:1084-1089): preprocessing applied plans['transpose_forward'].  `arr` is [Z,Y,X], or
    [C,Z,Y,X] whose channel axis stays in front"""
    if plans.get("transpose_forward") is None:
        return arr
    tb = list(plans.get("transpose_backward"))
    return np.ascontiguousarray(arr.transpose(tb if arr.ndim == 3 else [0] + [i + 1 for i in tb]))


def _timed_export(dev, **kwargs):
    t0 = time.perf_counter()
    torch.cuda.set_device(dev)                                                   # per-thread state: the resampling kernels must run on the caller's GPU
    save_segmentation_nifti_from_softmax(**kwargs)
    return time.perf_counter() - t0


def _submit_export(pool, trainer, export_kw, seg, softmax, npz, **kwargs):
    """One frame's export job.  softmax None: no resampling and no npz asked for, the probabilities never left the device and the frame is
    written from the device arg-max `seg`."""
    if npz is not None:
        kwargs["resampled_npz_fname"] = npz
    if softmax is not None:
        kwargs["segmentation_softmax"] = _to_file_axes(softmax, trainer.plans)
        # a region-based model: the labels of the (possibly resampled) probabilities follow the region rule, and the .pkl next to the npz
        # records the order (segmentation_export.py:141-150); None for every other model
        kwargs["region_class_order"] = getattr(trainer, "regions_class_order", None)
    else:                                        # (a region-based model's device labels are region labels already)
        kwargs.update(segmentation_softmax=None, seg_precomputed=_to_file_axes(seg, trainer.plans))
    return pool.apply_async(_timed_export, (trainer.device,), dict(export_kw, verbose=False, **kwargs))


def _export_flow_patient(result, trainer, output_filenames, property_list, export_kw, save_npz, pool):
    """predict.py:1084-1110 for one patient's device results: transpose back, submit one export job per frame to the pool.
    Returns (label files: every Segmentation/ file, then every Registered/ file; jobs)."""
    seg, softmax, flow, registered, _raw = result[:5]
    crop_out = result[5] if len(result) > 5 else None
    assert len(seg) == len(flow) == len(registered) and (softmax is None or len(softmax) == len(flow))
    if _VOXELMORPH_RAW is not None:
        assert crop_out is not None, "set_voxelmorph_raw was switched on after the device stage of this patient"
        write_raw(_VOXELMORPH_RAW[0], _VOXELMORPH_RAW[1], os.path.basename(_patient_folder(output_filenames)),
                  [os.path.basename(o)[:-7] for o in output_filenames], crop_out["softmax"], crop_out["flow"], crop_out["registered"], property_list,
                  crop_out["padding_need"], crop_out["size_before"], ed_position=0)
    seg_paths, reg_paths, jobs = [], [], []
    for t, out_fname in enumerate(output_filenames):
        seg_path, flow_path, reg_path = _flow_outputs(out_fname)
        seg_paths.append(seg_path)
        reg_paths.append(reg_path)
        jobs.append(_submit_export(pool, trainer, export_kw, seg[t], None if softmax is None else softmax[t], seg_path[:-7] + ".npz" if save_npz else None,
                                   out_fname=seg_path, properties_dict=property_list[t], flow=_to_file_axes(flow[t], trainer.plans), flow_path=flow_path,
                                   registered=_to_file_axes(registered[t], trainer.plans), registered_path=reg_path))
    return seg_paths + reg_paths, jobs


def _export_seg_patient(results, trainer, output_filenames, property_list, export_kw, save_npz, pool):
    """predict.py:962-997 for one patient's (seg, softmax or None) per frame: transpose back, one export job per frame writing
    `output_filenames[t]` (+ <case>.npz / .pkl with save_npz).  Returns (label files, jobs)."""
    jobs = [_submit_export(pool, trainer, export_kw, seg, softmax, output_filenames[t][:-7] + ".npz" if save_npz else None,
                           out_fname=output_filenames[t], properties_dict=property_list[t], properties_pkl=bool(save_npz))
            for t, (seg, softmax) in enumerate(results)]
    return list(output_filenames), jobs


def _finish_patient(label_paths, jobs, patient_folder, disable_postprocessing, model):
    """wait for a patient's export jobs, then predict.py:1139-1156 on its label files (largest-component filter when the model folder has a
    postprocessing.json, which is copied next to the patient's outputs).  Returns the seconds the export jobs worked."""
    work = sum(j.get() for j in jobs)
    if not disable_postprocessing:
        pp_file = join(model, "postprocessing.json")
        if os.path.isfile(pp_file):
            print("postprocessing...")
            shutil.copy(pp_file, patient_folder)
            for_which_classes, min_valid_obj_size = load_postprocessing(pp_file)
            for pth in label_paths:
                load_remove_save(pth, pth, for_which_classes, min_valid_obj_size)
        else:
            print("WARNING! Cannot run postprocessing because the postprocessing file is missing (%s)" % model)
    return work


def predict_flow(d, trainer, output_filenames, property_list, do_tta, mixed_precision, params, interpolation_order, force_separate_z,
                 interpolation_order_z, all_in_gpu, step_size, save_npz, disable_postprocessing, model, pool):
    """predict.py:1008-1162 for one patient: `d[t]` = preprocessed frame t (ED first), all frames form the cine sequence.
    Writes <patient>/{Segmentation,Flow,Registered}/<case>; returns the three path lists.
    After set_voxelmorph_raw(pred_path, pkl_path) the crop-space predictions are additionally written as `<pred_path>/Raw/...` +
    `<pkl_path>/<case>.pkl`, the input layout of voxelmorph_saver_* (cineflow.voxelmorph_saver)."""
    unlabeled = np.stack(d) + 1e-8                                               # predict.py:1025
    print("predicting", output_filenames)
    result = trainer.predict_preprocessed_data_return_seg_and_softmax_flow(
        unlabeled=unlabeled, target=None, target_mask=None, processor=trainer.processor, do_mirroring=do_tta,
        mirror_axes=trainer.data_aug_params["mirror_axes"], use_sliding_window=True, step_size=step_size, use_gaussian=True,
        all_in_gpu=all_in_gpu, mixed_precision=mixed_precision, verbose=False, return_crop=True)
    export_kw = {"force_separate_z": force_separate_z, "order": interpolation_order, "interpolation_order_z": interpolation_order_z}
    label_paths, jobs = _export_flow_patient(result, trainer, output_filenames, property_list, export_kw, save_npz, pool)
    print("inference done. Now waiting for the segmentation export to finish...")
    _finish_patient(label_paths, jobs, _patient_folder(output_filenames), disable_postprocessing, model)
    outputs = [_flow_outputs(o) for o in output_filenames]
    return [o[0] for o in outputs], [o[1] for o in outputs], [o[2] for o in outputs]


def predict_non_flow(d, trainer, output_filenames, property_list, do_tta, mixed_precision, params, interpolation_order, force_separate_z,
                     interpolation_order_z, all_in_gpu, step_size, save_npz, disable_postprocessing, model, pool):
    """predict.py:926-1005: segmentation only, sliding window + TTA; the softmax of every frame is the mean over the folds in `params`
    (what :952-960 intend; as written :955 passes the frame list and only the first frame is reached).  All folds are made resident once
    (`load_ensemble`), all frames go through predict_cine_2Dconv_tiled in one call.  Returns the export jobs."""
    if getattr(trainer, "_ensemble_of", None) is not params:
        trainer.load_ensemble(params)
        trainer._ensemble_of = params
    print("predicting", output_filenames)
    results = trainer.predict_volumes_seg(list(d), do_mirroring=do_tta, step_size=step_size, mixed_precision=mixed_precision)
    export_kw = {"force_separate_z": force_separate_z, "order": interpolation_order, "interpolation_order_z": interpolation_order_z}
    return _export_seg_patient(results, trainer, output_filenames, property_list, export_kw, save_npz, pool)[1]


def _groups(items, max_slices, first_slices):
    """The device batches of the file-level API: `items` yields (item, nslices) in patient order, lists of items come out.  An item joins
    the group unless the group is non-empty and would then hold more than `cap` slices (so one larger than the cap goes alone).
    The first device batch is small (`first_slices`) and the cap doubles from batch to batch up to `max_slices`: the device starts as soon
    as two or so patients are read instead of waiting for a full batch of 64 slices, and the later patients are preprocessed behind it.
    Exactly one item beyond a group has been pulled when that group is yielded, and none further."""
    cap = min(max_slices, first_slices)
    group, nslices = [], 0
    for item, z in items:
        if group and nslices + z > cap:
            yield group
            cap = min(max_slices, 2 * cap)
            group, nslices = [], 0
        group.append(item)
        nslices += z
    if group:
        yield group


def _predict_patients(model, cases, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save, do_tta, mixed_precision, all_in_gpu,
                      step_size, checkpoint_name, segmentation_export_kwargs, disable_postprocessing, max_slices=None):
    """predict.py:228-354 + :1008-1110 for a LIST of patients (`cases[i]` = (list_of_lists, output_filenames, ed_index)): the model is loaded
    once, frames are read and preprocessed by a thread pool one group of patients ahead, every group's cropped slices (up to `max_slices`)
    share one device batch, and finished patients are exported by the NIfTI pool while the next group is on the device.
    A segmentation-only model (trainer.flow_net is None) takes the reference's other branch (predict.py:320-353 -> predict_non_flow) inside the
    same pipeline: all frames of all patients of a group go through predict_cine_2Dconv_tiled's device path in one call, every frame is
    written to `output_filenames[t]` itself, nothing under Flow/ or Registered/; ED index, voxelmorph_raw and Processor are not used.
    A case may carry a fourth entry, `segs_from_prev_stage` (one label file per frame, or None): it goes to preprocess_patient with its frame, so
    the labels are resized and encoded on the preprocessing thread's stream (predict.py:302 -> :61-85)."""
    t_start = time.perf_counter()
    max_slices = max_slices or MAX_SLICES_PER_LAUNCH
    # the calling thread issues ~1500 kernel launches per device batch from Python while up to 32 pool threads read, crop and compress: with
    # the interpreter's default 5 ms switch interval every hand-over of the GIL to a pool thread could stall the launch stream for
    # milliseconds (device time of the 16-patient API bench 6.4 -> 10.4 s once preprocessing overlapped fully, profiles/r03_api_split.md)
    switch_prev = sys.getswitchinterval()
    trainer, params = _cached_model(model, folds, mixed_precision, checkpoint_name)
    timing = {"load_s": time.perf_counter() - t_start, "preprocess_wait_s": 0.0, "preprocess_work_s": 0.0, "device_s": 0.0, "export_wait_s": 0.0,
              "export_work_s": 0.0, "device_batches": 0, "patients": len(cases), "frames": 0, "slices": 0}
    export_kw = _export_kwargs(trainer, segmentation_export_kwargs)
    seg_only = trainer.flow_net is None
    export_patient = _export_seg_patient if seg_only else _export_flow_patient
    orders = []
    for list_of_lists, output_filenames, ed_index, *prev in cases:
        assert len(list_of_lists) == len(output_filenames)
        if prev and prev[0] is not None:
            assert len(prev[0]) == len(output_filenames)
        trainer.check_prev_stage(bool(prev) and prev[0] is not None)
        for o in output_filenames:
            for sub in ((None,) if seg_only else ("Segmentation", "Flow", "Registered")):
                os.makedirs(join(os.path.dirname(o), sub) if sub else os.path.dirname(os.path.abspath(o)), exist_ok=True)
        T = len(list_of_lists)
        if seg_only:
            orders.append(list(range(T)))                                        # frames are independent: no ED rotation
        else:
            orders.append(list(range(ed_index, T)) + list(range(0, ed_index)))  # ED first (put_ed_first, predict.py:1165-1193)

    tls = threading.local()
    stream_ids = itertools.count()

    def pre_one(files, seg_prev=None):
        # every preprocessing thread issues its (small) device kernels on a HIP stream of its own: on the default stream they -- and the
        # host read-backs between them -- queued behind the seconds-long network batch of the main thread.  The streams are taken from a
        # process-wide pool (thread k of every call gets stream k): torch's caching allocator keeps one pool of blocks per stream, so fresh
        # streams in every call meant fresh hipMalloc calls -- each a device-wide synchronisation -- under the running network batch
        t0 = time.perf_counter()
        if not hasattr(tls, "stream"):
            torch.cuda.set_device(trainer.device)                                # the current device is per thread (a new thread starts on GPU 0)
            tls.stream = _pooled_stream(trainer.device, next(stream_ids))
        with torch.cuda.stream(tls.stream):
            r = trainer.preprocess_patient(files) if seg_prev is None else trainer.preprocess_patient(files, seg_prev)   # predict.py:302
            tls.stream.synchronize()
        return r, time.perf_counter() - t0

    pre_pool = ThreadPool(max(1, num_threads_preprocessing))
    pool = ThreadPool(max(1, num_threads_nifti_save))
    submitted = deque()                                                          # (case index, [async results per frame])
    nxt = 0
    # slices of a patient are only known after preprocessing; groups are filled greedily in patient order.  The pool runs `ahead` patients
    # in front of the collector: at least one whole device batch more than the group being assembled, so that the frames of the NEXT
    # group are read and cropped while this one is on the device (with 4 the second half of the next group was only submitted after
    # the device batch had finished: 3.4 of 10.5 s of the 16-patient API bench were spent waiting for it, profiles/r03_api_split.md).
    # Reading and preprocessing the whole request before the first device batch was slower: the networks then ran at their device-only
    # rate (5.6 instead of 8.1 s for 16 patients) but the reading was not hidden (4.9 s), 310 against 361 frames/s (same profile).
    ahead = 8

    def submit_more():
        nonlocal nxt
        while nxt < len(cases) and len(submitted) < ahead:
            lol = cases[nxt][0]
            prev = cases[nxt][3] if len(cases[nxt]) > 3 and cases[nxt][3] is not None else [None] * len(lol)
            submitted.append((nxt, [pre_pool.apply_async(pre_one, (lol[i], prev[i])) for i in orders[nxt]]))
            nxt += 1

    def preprocessed():
        """((case index, its preprocessed frames), slices) of the next patient, in order: waits for its frames, accounts the wait"""
        while submitted:
            ci, asyncs = submitted.popleft()
            t0 = time.perf_counter()
            got = [a.get() for a in asyncs]
            timing["preprocess_wait_s"] += time.perf_counter() - t0
            timing["preprocess_work_s"] += sum(g[1] for g in got)
            submit_more()
            yield (ci, [g[0] for g in got]), got[0][0][0].shape[1]

    finishing = deque()                                                          # exports in flight: (label files, jobs, patient folder)

    sys.setswitchinterval(GIL_SWITCH_INTERVAL)                                   # restored in the finally below
    try:
        submit_more()
        for group in _groups(preprocessed(), max_slices, FIRST_BATCH_SLICES):
            t0 = time.perf_counter()
            nslices = sum(pre[0][0].shape[1] for _ci, pre in group)
            print("predicting %d patient(s), %d slices in one device batch" % (len(group), nslices))
            ahead = max(ahead, 2 * len(group) + 2)
            submit_more()
            # the probabilities come to the host only if the exporter needs them: for the npz, or to resample them back to the size
            # before the preprocessing's resampling (segmentation_export.py:84-127); otherwise it writes the device arg-max
            tf_ = list(trainer.plans["transpose_forward"])
            resampled = any(tuple(p_[0].shape[1:]) != tuple(np.array(p_[2]["size_after_cropping"])[tf_]) for _ci, pre in group for p_ in pre)
            want_softmax = bool(save_npz or resampled)
            if seg_only:
                flat = iter(trainer.predict_volumes_seg([p_[0] for _ci, pre in group for p_ in pre], do_mirroring=do_tta, step_size=step_size,
                                                        mixed_precision=mixed_precision, want_softmax=want_softmax))
                results = [list(itertools.islice(flat, len(pre))) for _ci, pre in group]
            else:
                unl = [np.stack([p_[0] for p_ in pre]) + 1e-8 for _ci, pre in group]      # predict.py:1025
                # the crop-space copies only when the voxelmorph_saver tree is being written; the `raw` tensor (frames + crop-space flow) the
                # reference returns for its trainer's plots is not consumed by the exporter
                results = trainer.predict_patients_flow(unl, do_mirroring=do_tta, mirror_axes=trainer.data_aug_params["mirror_axes"],
                                                        return_crop=_VOXELMORPH_RAW is not None, want_raw=False, want_softmax=want_softmax)
            torch.cuda.synchronize()
            timing["device_s"] += time.perf_counter() - t0
            timing["device_batches"] += 1
            timing["slices"] += nslices
            for (ci, pre), res in zip(group, results):
                outs = [cases[ci][1][i] for i in orders[ci]]
                timing["frames"] += len(outs)
                finishing.append(export_patient(res, trainer, outs, [p_[2] for p_ in pre], export_kw, save_npz, pool) + (_patient_folder(outs),))
            while len(finishing) > 2 * max(1, len(group)):                       # bound the host memory held by queued exports
                t0 = time.perf_counter()
                timing["export_work_s"] += _finish_patient(*finishing.popleft(), disable_postprocessing, model)
                timing["export_wait_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        while finishing:
            timing["export_work_s"] += _finish_patient(*finishing.popleft(), disable_postprocessing, model)
        timing["export_wait_s"] += time.perf_counter() - t0
    except BaseException:
        # a failed batch must not wait for every queued preprocessing / export job: drop them
        pre_pool.terminate()
        pool.terminate()
        raise
    finally:
        pre_pool.close()                                                         # (no-ops after terminate())
        pool.close()
        pre_pool.join()
        pool.join()
        sys.setswitchinterval(switch_prev)
    timing["total_s"] = time.perf_counter() - t_start
    if API_PROFILE:
        timing.update({"device_" + k: v for k, v in DEVICE_SPLIT.items()})
        DEVICE_SPLIT.clear()
    LAST_TIMING.clear()
    LAST_TIMING.update(timing)
    if seg_only:
        return [list(c[1]) for c in cases]                                       # the written label files, per patient
    return [[_flow_outputs(o) for o in c[1]] for c in cases]


def predict_cases(model, list_of_lists, output_filenames, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save,
                  segs_from_prev_stage=None, do_tta=True, mixed_precision=True, overwrite_existing=False, all_in_gpu=False,
                  step_size=0.5, checkpoint_name="model_final_checkpoint", segmentation_export_kwargs=None,
                  disable_postprocessing=False, ed_index=0):
    """predict.py:228-354 for ONE patient: `list_of_lists[t]` = the modality files of frame t.  All frames form the cine
    sequence; frame `ed_index` is rotated to the front for the ED-anchored recurrence (put_ed_first, :1165-1193)."""
    assert len(list_of_lists) == len(output_filenames)
    if segs_from_prev_stage is not None:
        assert len(segs_from_prev_stage) == len(output_filenames)
    return _predict_patients(model, [(list_of_lists, output_filenames, ed_index, segs_from_prev_stage)], folds, save_npz, num_threads_preprocessing, num_threads_nifti_save,
                             do_tta, mixed_precision, all_in_gpu, step_size, checkpoint_name, segmentation_export_kwargs, disable_postprocessing)[0]


def predict_cases_fast(model, list_of_lists, output_filenames, folds, num_threads_preprocessing, num_threads_nifti_save,
                       segs_from_prev_stage=None, do_tta=True, mixed_precision=True, overwrite_existing=False, all_in_gpu=False,
                       step_size=0.5, checkpoint_name="model_final_checkpoint", segmentation_export_kwargs=None,
                       disable_postprocessing=False):
    """predict.py:356-501 ("fast": no resampled-softmax npz).  Everything already stays on the GPU here, so this is
    predict_cases with save_npz=False."""
    return predict_cases(model, list_of_lists, output_filenames, folds, False, num_threads_preprocessing, num_threads_nifti_save,
                         segs_from_prev_stage, do_tta, mixed_precision, overwrite_existing, all_in_gpu, step_size, checkpoint_name,
                         segmentation_export_kwargs, disable_postprocessing)


def predict_cases_fastest(model, list_of_lists, output_filenames, folds, num_threads_preprocessing, num_threads_nifti_save,
                          segs_from_prev_stage=None, do_tta=True, mixed_precision=True, overwrite_existing=False, all_in_gpu=False,
                          step_size=0.5, checkpoint_name="model_final_checkpoint", disable_postprocessing=False):
    """predict.py:504-626 ("fastest": argmax on the device, nearest-neighbour export)."""
    return predict_cases(model, list_of_lists, output_filenames, folds, False, num_threads_preprocessing, num_threads_nifti_save,
                         segs_from_prev_stage, do_tta, mixed_precision, overwrite_existing, all_in_gpu, step_size, checkpoint_name,
                         {"force_separate_z": None, "interpolation_order": 0, "interpolation_order_z": 0}, disable_postprocessing)


def lowres_segmentation_file(lowres_segmentations, patient, case_id):
    """the previous stage's label file of one case: `<l>/<patient>/<case>.nii.gz` (what a segmentation-only predict_from_folder run writes)
    when it exists, else `<l>/<case>.nii.gz` (predict.py:730)"""
    own = join(lowres_segmentations, patient, case_id + ".nii.gz")
    return own if os.path.isfile(own) else join(lowres_segmentations, case_id + ".nii.gz")


def predict_from_folder(model, input_folder, output_folder, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save,
                        lowres_segmentations, part_id, num_parts, tta, mixed_precision=True, overwrite_existing=True, mode="normal",
                        overwrite_all_in_gpu=None, step_size=0.5, checkpoint_name="model_final_checkpoint",
                        segmentation_export_kwargs=None, disable_postprocessing=False):
    """predict.py:665-780.  Patients are sharded `patients[part_id::num_parts]` (one process per GPU); every patient of
    the shard is processed.  Returns {patient: per frame (Segmentation, Flow, Registered) paths}; for a segmentation-only model folder
    (plans.json without 'flow_net') {patient: the written `<out>/<patient>/<case>.nii.gz` paths}.  (set_voxelmorph_raw / the CLI's --voxelmorph_raw additionally produce the voxelmorph_saver input tree;
    the argument list itself is the reference's, name for name.)
    lowres_segmentations (predict.py:728-733): the folder with the previous stage's label files, for a cascade model.  Per case
    `<l>/<patient>/<case>.nii.gz` is taken when it exists -- the layout a segmentation-only run of this function writes, so the output folder
    of the lowres run is passed as it is -- else `<l>/<case>.nii.gz`, the reference's literal join.  Missing files, a non-directory, a cascade
    model without the folder and a folder given to another model all raise before the checkpoint is read."""
    os.makedirs(output_folder, exist_ok=True)
    assert os.path.isfile(join(model, "plans.json")), "Folder with saved model weights must contain a plans.json file"
    shutil.copy(join(model, "plans.json"), output_folder)
    with open(join(model, "plans.json")) as f:
        model_plans = json.load(f)
    expected_num_modalities = model_plans["num_modalities"]
    if lowres_segmentations is not None:
        assert os.path.isdir(lowres_segmentations), "if lowres_segmentations is not None then it must point to a directory"
    _check_prev_stage((model_plans.get("seg_net") or {}).get("prev_stage_classes"), lowres_segmentations is not None, model)
    if mode not in ("normal", "fast", "fastest"):
        raise ValueError("unrecognized mode. Must be normal, fast or fastest")
    patients = sorted(p for p in os.listdir(input_folder) if os.path.isdir(join(input_folder, p)))
    # one process per GPU under torchrun (RANK / WORLD_SIZE): the reference's partition with part_id = rank, num_parts = world unless the
    # caller partitions explicitly (predict.py:743, :806-821)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and num_parts == 1:
        part_id, num_parts = int(os.environ.get("RANK", "0")), world
    shard, cases = patients[part_id::num_parts], []
    for patient in shard:
        current_input_folder = join(input_folder, patient)
        current_output_folder = join(output_folder, patient)
        case_ids = check_input_folder_and_return_caseIDs(current_input_folder, expected_num_modalities)
        output_files = [join(current_output_folder, i + ".nii.gz") for i in case_ids]
        all_files = subfiles(current_input_folder, suffix=".nii.gz", join_=False, sort=True)
        list_of_lists = [[join(current_input_folder, i) for i in all_files if i[:len(j)].startswith(j) and len(i) == (len(j) + 12)]
                         for j in case_ids]
        ed_index = 0
        csv_path = join(current_input_folder, patient + ".csv")                  # predict.py:700, :1196-1198
        if os.path.isfile(csv_path):
            ed_index = get_ed_es_indices(csv_path)[0]
        prev = None
        if lowres_segmentations is not None:
            prev = [lowres_segmentation_file(lowres_segmentations, patient, i) for i in case_ids]
            assert all([os.path.isfile(i) for i in prev]), "not all lowres_segmentations files are present. " \
                                                           "(I was searching for case_id.nii.gz in that folder)"
        cases.append((list_of_lists, output_files, ed_index, prev))
    seg_exp = segmentation_export_kwargs
    if mode != "normal":
        assert save_npz is False                                                 # predict.py:755, :771
    if mode == "fastest":                                                        # predict.py:504-626: nearest-neighbour export
        seg_exp = {"force_separate_z": None, "interpolation_order": 0, "interpolation_order_z": 0}
    if not cases and world > 1:
        _cached_model(model, folds, mixed_precision, checkpoint_name)            # an empty shard still takes part in the weight broadcast
    res = _predict_patients(model, cases, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save, tta, mixed_precision,
                            bool(overwrite_all_in_gpu), step_size, checkpoint_name, seg_exp, disable_postprocessing) if cases else []
    return dict(zip(shard, res))


def main(argv=None):
    """CLI flags of predict.py:782-858 / predict_simple.py:34-131."""
    parser = argparse.ArgumentParser()
    parser.add_argument("-i", "--input_folder", required=True)
    parser.add_argument("-o", "--output_folder", required=True)
    parser.add_argument("-m", "--model_output_folder", required=True)
    parser.add_argument("-f", "--folds", nargs="+", default="None")
    parser.add_argument("-z", "--save_npz", required=False, action="store_true")
    parser.add_argument("-l", "--lowres_segmentations", required=False, default="None")
    parser.add_argument("--lowres_model", required=False, default=None, help="model folder of the cascade's 3d_lowres stage: without -l it is "
                        "predicted first into <output_folder>/3d_lowres_predictions, which then serves as -l (predict_simple.py:196-215)")
    parser.add_argument("--part_id", type=int, required=False, default=0)
    parser.add_argument("--num_parts", type=int, required=False, default=1)
    parser.add_argument("--num_threads_preprocessing", required=False, default=6, type=int)
    parser.add_argument("--num_threads_nifti_save", required=False, default=2, type=int)
    parser.add_argument("--tta", required=False, type=int, default=1)
    parser.add_argument("--disable_tta", required=False, default=False, action="store_true")
    parser.add_argument("--overwrite_existing", required=False, type=int, default=1)
    parser.add_argument("--mode", type=str, default="normal", required=False)
    parser.add_argument("--all_in_gpu", type=str, default="None", required=False)
    parser.add_argument("--step_size", type=float, default=0.5, required=False)
    parser.add_argument("--disable_mixed_precision", default=False, action="store_true", required=False)
    parser.add_argument("-chk", default="model_final_checkpoint", required=False)
    parser.add_argument("--voxelmorph_raw", default=None, required=False, help="also write <dir>/Raw/{Registered,Segmentation,Flow}/<patient>/ "
                        "(crop-space predictions, the input of voxelmorph_saver_*)")
    parser.add_argument("--voxelmorph_pkl", default=None, required=False, help="folder for the per-file .pkl properties (default <voxelmorph_raw>/pkl)")
    a = parser.parse_args(argv)
    folds = a.folds if a.folds != "None" and a.folds != ["None"] else None
    if isinstance(folds, list):
        folds = [int(i) if i != "all" else i for i in folds]
    all_in_gpu = None if a.all_in_gpu == "None" else a.all_in_gpu == "True"
    tta = bool(a.tta) and not a.disable_tta
    if a.voxelmorph_raw is not None:
        set_voxelmorph_raw(a.voxelmorph_raw, a.voxelmorph_pkl)
    lowres = None if a.lowres_segmentations == "None" else a.lowres_segmentations
    if a.lowres_model is not None and lowres is None:
        print("lowres_segmentations is None. Attempting to predict 3d_lowres first...")
        assert a.part_id == 0 and a.num_parts == 1, "if you don't specify a --lowres_segmentations folder for the " \
                                                    "inference of the cascade, custom values for part_id and num_parts " \
                                                    "are not supported. If you wish to have multiple parts, please " \
                                                    "run the 3d_lowres inference first (separately)"
        assert os.path.isdir(a.lowres_model), "model output folder not found. Expected: %s" % a.lowres_model
        lowres = join(a.output_folder, "3d_lowres_predictions")
        predict_from_folder(a.lowres_model, a.input_folder, lowres, folds, False, a.num_threads_preprocessing, a.num_threads_nifti_save, None,
                            a.part_id, a.num_parts, tta, mixed_precision=not a.disable_mixed_precision,
                            overwrite_existing=bool(a.overwrite_existing), mode=a.mode, overwrite_all_in_gpu=all_in_gpu, step_size=a.step_size,
                            checkpoint_name=a.chk)
        print("3d_lowres done")
    return predict_from_folder(a.model_output_folder, a.input_folder, a.output_folder, folds, a.save_npz, a.num_threads_preprocessing,
                               a.num_threads_nifti_save, lowres, a.part_id, a.num_parts, tta, mixed_precision=not a.disable_mixed_precision,
                               overwrite_existing=bool(a.overwrite_existing), mode=a.mode, overwrite_all_in_gpu=all_in_gpu,
                               step_size=a.step_size, checkpoint_name=a.chk)


if __name__ == "__main__":
    main()
