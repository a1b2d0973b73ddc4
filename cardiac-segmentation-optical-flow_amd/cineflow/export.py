"""NIfTI / NPZ export of predicted volumes (segmentation_export.py) and the largest-component post-processing
(connected_components.py), with the resampling and the component labelling on the device (cineflow.ops)."""
import ast
import json
import os
import pickle

import numpy as np
import torch

from . import ops
from .folder_io import subfiles                                    # noqa: F401  (the old import path)
from .nifti import read_nifti, write_nifti

join = os.path.join

RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3   # nnunet/configuration.py


def get_do_separate_z(spacing, anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """preprocessing.py:30-32."""
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(new_spacing):
    """preprocessing.py:35-37."""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def probabilities_as_stored(probs, region_class_order=None):
    """The fp16 array a `-z` run stores.  Softmax models: numpy's round-to-nearest, as the reference stores it.  Region models paint a label
    where p > 0.5, and fp16 has no value between 0.5 and 0.5 + 2^-11: round-to-nearest turns every p in (0.5, 0.5 + 2^-12] into 0.5, which
    is no longer `> 0.5`, so the stored member would contradict the label file written from the same probabilities (on a seeded 3-D case 21
    of 5376 voxels).  Those values alone are rounded UP to the next fp16 instead (0.5 + 2^-11: one unit in the last place instead of a
    half); nothing at or below 0.5 can round above it, 0.5 being an fp16 value.  So `stored > 0.5` exactly where `p > 0.5`, and
    cineflow.ensemble_predictions on a folder and its copy writes the folder's own label files."""
    stored = probs.astype(np.float16)
    if region_class_order is not None:
        half = np.float16(0.5)
        stored[(probs > 0.5) & (stored <= half)] = np.nextafter(half, np.float16(1))
    return stored


def save_segmentation_nifti_from_softmax(segmentation_softmax, out_fname, properties_dict, order=1, region_class_order=None,
                                         seg_postprogess_fn=None, seg_postprocess_args=None, resampled_npz_fname=None,
                                         non_postprocessed_fname=None, force_separate_z=None, interpolation_order_z=0, verbose=True,
                                         flow=None, flow_path=None, registered=None, registered_path=None, seg_precomputed=None,
                                         properties_pkl=False, compress="zlib"):
    """segmentation_export.py:29-223: resample softmax / flow / registered labels back to the size before resampling (device
    kernels, cineflow.ops.resample_data_or_seg), rescale the flow to the new pixel grid, argmax, place into the crop bounding
    box, write uint8 NIfTI with the case's geometry; flow [2,Z,Y,X] -> npz `flow` [Y,X,Z,2] float32 + `spacing`.
    properties_pkl: also write the properties next to the npz as `<npz name>.pkl` (segmentation_export.py:143; the segmentation-only route)."""
    if isinstance(segmentation_softmax, str):
        assert os.path.isfile(segmentation_softmax), "If isinstance(segmentation_softmax, str) then isfile(segmentation_softmax) must be True"
        del_file = segmentation_softmax
        segmentation_softmax = np.load(segmentation_softmax)
        os.remove(del_file)
    shape_after_crop = tuple(properties_dict.get("size_after_cropping"))
    if seg_precomputed is not None:
        # the caller already holds arg-max(softmax) at the size after cropping (computed on the device, first maximum like numpy) and needs
        # neither the resampling branch nor the npz: the probabilities never left the device
        assert segmentation_softmax is None and resampled_npz_fname is None and region_class_order is None
        assert tuple(seg_precomputed.shape) == shape_after_crop, "seg_precomputed must have the size after cropping"
        current_shape = (0,) + tuple(seg_precomputed.shape)
    else:
        current_shape = segmentation_softmax.shape
    shape_before_crop = properties_dict.get("original_size_of_raw_data")
    if any(i != j for i, j in zip(current_shape[1:], shape_after_crop)):
        if force_separate_z is None:                                             # segmentation_export.py:88-98
            if get_do_separate_z(properties_dict.get("original_spacing")):
                do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get("original_spacing"))
            elif get_do_separate_z(properties_dict.get("spacing_after_resampling")):
                do_separate_z, lowres_axis = True, get_lowres_axis(properties_dict.get("spacing_after_resampling"))
            else:
                do_separate_z, lowres_axis = False, None
        else:
            do_separate_z = force_separate_z
            lowres_axis = get_lowres_axis(properties_dict.get("original_spacing")) if do_separate_z else None
        if lowres_axis is not None and len(lowres_axis) != 1:
            do_separate_z = False
        if verbose:
            print("separate z:", do_separate_z, "lowres axis", lowres_axis)
        seg_old_spacing = ops.resample_data_or_seg(segmentation_softmax, shape_after_crop, is_seg=False, axis=lowres_axis, order=order,
                                                   do_separate_z=do_separate_z, order_z=interpolation_order_z)
        if flow is not None:
            rescale_y = shape_after_crop[1] / flow.shape[2]
            rescale_x = shape_after_crop[2] / flow.shape[3]
            flow = ops.resample_data_or_seg(np.asarray(flow, np.float32), shape_after_crop, is_seg=False, axis=lowres_axis, order=order,
                                            do_separate_z=do_separate_z, order_z=interpolation_order_z)
            flow[0] = flow[0] * rescale_y                                        # segmentation_export.py:123-124
            flow[1] = flow[1] * rescale_x
        if registered is not None:
            registered = ops.resample_data_or_seg(np.asarray(registered), shape_after_crop, is_seg=True, axis=lowres_axis, order=0,
                                                  do_separate_z=do_separate_z, order_z=0)
    else:
        if verbose:
            print("no resampling necessary")
        seg_old_spacing = segmentation_softmax
    if resampled_npz_fname is not None:
        if compress == "zlib":
            np.savez_compressed(resampled_npz_fname, softmax=probabilities_as_stored(seg_old_spacing, region_class_order))
        else:                                                                    # (the device deflates; the file holds the same array)
            from . import deflate
            deflate.check_compress(compress)
            deflate.savez_compressed(resampled_npz_fname, softmax=probabilities_as_stored(seg_old_spacing, region_class_order))
        if region_class_order is not None:                                       # segmentation_export.py:141-142: an ensemble member says so itself
            properties_dict["regions_class_order"] = region_class_order
        if properties_pkl:
            with open(resampled_npz_fname[:-4] + ".pkl", "wb") as f:
                pickle.dump(properties_dict, f)
    if seg_precomputed is not None:
        seg = np.asarray(seg_precomputed)
    elif region_class_order is None:
        seg = seg_old_spacing.argmax(0)
    else:
        seg = np.zeros(seg_old_spacing.shape[1:])
        for i, c in enumerate(region_class_order):
            seg[seg_old_spacing[i] > 0.5] = c
    bbox = properties_dict.get("crop_bbox")
    if bbox is not None:                                                         # segmentation_export.py:153-177
        bbox = [list(b) for b in bbox]
        for c in range(3):
            bbox[c][1] = int(np.min((bbox[c][0] + seg.shape[c], shape_before_crop[c])))
        sl = tuple(slice(b[0], b[1]) for b in bbox)
        full = np.zeros(shape_before_crop, dtype=np.uint8)
        full[sl] = seg
        seg = full
        if flow is not None:
            f_full = np.zeros([2] + list(shape_before_crop), dtype=np.float32)
            f_full[(slice(None),) + sl] = flow
            flow = f_full
        if registered is not None:
            r_full = np.zeros(shape_before_crop, dtype=np.uint8)
            r_full[sl] = registered[0]
            registered = r_full[None]
    if seg_postprogess_fn is not None:
        seg = seg_postprogess_fn(np.copy(seg), *seg_postprocess_args)
    geo = (properties_dict["itk_spacing"], properties_dict["itk_origin"], properties_dict["itk_direction"])
    write_nifti(out_fname, seg.astype(np.uint8), *geo)
    if flow is not None:
        np.savez(flow_path, flow=np.asarray(flow, np.float32).transpose(2, 3, 1, 0), spacing=properties_dict["itk_spacing"])
    if registered is not None:
        write_nifti(registered_path, np.asarray(registered[0]).astype(np.uint8), *geo)


# ------------------------------------------------------------------------------------------------ post-processing
def load_postprocessing(json_file):
    """connected_components.py:109-120."""
    with open(json_file) as f:
        a = json.load(f)
    mv = ast.literal_eval(a["min_valid_object_sizes"]) if "min_valid_object_sizes" in a else None
    return a["for_which_classes"], mv


def load_remove_save(input_file, output_file, for_which_classes, minimum_valid_object_size=None):
    """connected_components.py:31-48: keep the largest connected component of each class (device kernels, cineflow.ops)."""
    img, props = read_nifti(input_file)
    volume_per_voxel = float(np.prod(props["itk_spacing"], dtype=np.float64))
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8))).to(dev)
    fw = [tuple(c) if isinstance(c, list) else c for c in for_which_classes] if for_which_classes is not None else None
    mv = None
    if minimum_valid_object_size is not None:
        mv = {(tuple(k) if isinstance(k, list) else k): v for k, v in minimum_valid_object_size.items()}
    t, largest_removed, kept_size = ops.remove_all_but_the_largest_connected_component(t, fw, volume_per_voxel, mv)
    write_nifti(output_file, t.cpu().numpy(), props["itk_spacing"], props["itk_origin"], props["itk_direction"])
    return largest_removed, kept_size
