"""Test-time preprocessing on the device -- the caller side of the hot path.

Mirrors the reference interface of nnunet/preprocessing/cropping.py and nnunet/preprocessing/preprocessing.py (same function and
class names, argument meaning and return values; numpy in, numpy out like the reference, device tensors kept when given) so that
`trainer.preprocess_patient` (nnunet/training/network_training/nnUNetTrainer.py:571-597) is a drop-in.  Every number comes from
libcineflow_hip.so (csrc/preprocess.hip, csrc/postprocess.hip); torch only holds memory, slices and moves it.
"""
import copy
import ctypes
import os
import pickle
import shutil
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from ._lib import check, lib
from .nifti import read_nifti
from .ops import _f32, _stream, _u8

RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3  # nnunet/configuration.py


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a, dtype=torch.float32):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(_dev(), dtype=dtype).contiguous()


# ------------------------------------------------------------------------------------------------ cropping.py
def create_nonzero_mask(data):
    """cropping.py:25-32: OR over the modalities of data != 0, then scipy's binary_fill_holes.  data (C, X, Y, Z) or (C, X, Y);
    returns a bool array of the same kind (numpy / device tensor) as `data`."""
    was_numpy = not torch.is_tensor(data)
    t = _to_dev(data)
    assert t.dim() in (3, 4), "data must have shape (C, X, Y, Z) or shape (C, X, Y)"
    C = t.shape[0]
    shape = tuple(t.shape[1:])
    D, H, W = (1,) * (3 - len(shape)) + shape
    n = D * H * W
    mask = torch.empty(n, dtype=torch.uint8, device=t.device)
    check(lib().cf_nonzero_mask(_f32(t), C, n, _u8(mask), _stream()), "cf_nonzero_mask")
    # background components by the connected-component sweeps of the export step, then the hole fill
    labels = torch.empty(n, dtype=torch.int32, device=t.device)
    changed = torch.zeros(1, dtype=torch.int32, device=t.device)
    zero = (ctypes.c_uint8 * 1)(0)
    check(lib().cf_cc_init(_u8(mask), labels.data_ptr(), n, ctypes.cast(zero, ctypes.c_void_p), 1, _stream()), "cf_cc_init")
    while True:
        changed.zero_()
        for _ in range(8):
            check(lib().cf_cc_sweep(labels.data_ptr(), D, H, W, changed.data_ptr(), _stream()), "cf_cc_sweep")
        if int(changed.item()) == 0:
            break
    touch = torch.empty(n, dtype=torch.int32, device=t.device)
    check(lib().cf_fill_holes(_u8(mask), labels.data_ptr(), touch.data_ptr(), D, H, W, len(shape), _stream()), "cf_fill_holes")
    out = mask.view(shape).bool()
    return out.cpu().numpy() if was_numpy else out


def get_bbox_from_mask(mask, outside_value=0):
    """cropping.py:47-55 -> [[minz, maxz+1], [minx, maxx+1], [miny, maxy+1]] as Python ints."""
    t = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
    t = (t != outside_value).to(_dev(), dtype=torch.uint8).contiguous()
    assert t.dim() == 3, "only supports 3d images"
    bbox = torch.empty(6, dtype=torch.int32, device=t.device)
    check(lib().cf_mask_bbox(_u8(t), t.shape[0], t.shape[1], t.shape[2], bbox.data_ptr(), _stream()), "cf_mask_bbox")
    b = bbox.cpu().tolist()
    if b[1] < 0:
        raise ValueError("get_bbox_from_mask: the mask is empty")   # np.min of an empty sequence raises in the reference
    return [[b[0], b[1] + 1], [b[2], b[3] + 1], [b[4], b[5] + 1]]


def crop_to_bbox(image, bbox):
    """cropping.py:58-61."""
    assert len(image.shape) == 3, "only supports 3d images"
    return image[bbox[0][0]:bbox[0][1], bbox[1][0]:bbox[1][1], bbox[2][0]:bbox[2][1]]


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py:104-137 -> (data, seg, bbox); seg is created (0 inside the mask, nonzero_label outside; all 0 for a positive label,
    as the reference leaves it) when absent."""
    was_numpy = not torch.is_tensor(data)
    t = _to_dev(data)
    nonzero_mask = create_nonzero_mask(t)
    bbox = get_bbox_from_mask(nonzero_mask, 0)
    sl = (slice(None), slice(*bbox[0]), slice(*bbox[1]), slice(*bbox[2]))
    t = t[sl].contiguous()
    m = nonzero_mask[sl[1:]].to(torch.uint8).contiguous()
    # a created segmentation is the zero map with `nonzero_label` outside the mask (cropping.py:131-135)
    s = _to_dev(seg)[sl].contiguous() if seg is not None else torch.zeros((1,) + tuple(m.shape), dtype=torch.float32, device=t.device)
    # (the reference builds a created segmentation as mask -> label outside -> `[> 0] = 0`: a positive label leaves it all zero)
    if seg is not None or nonzero_label <= 0:
        check(lib().cf_seg_outside_mask(_f32(s), _u8(m), s.shape[0], m.numel(), float(nonzero_label), _stream()), "cf_seg_outside_mask")
    seg_dtype = seg.dtype if seg is not None else (np.int64 if was_numpy else torch.int64)
    if was_numpy:
        return t.cpu().numpy(), s.cpu().numpy().astype(seg_dtype), bbox
    return t, s.to(seg_dtype), bbox


def load_case_from_list_of_files(data_files, seg_file=None, info_dict=None):
    """cropping.py:74-101 with the package's NIfTI-1 reader in place of SimpleITK (absent from the image)."""
    assert isinstance(data_files, (list, tuple)), "case must be either a list or a tuple"
    properties = OrderedDict()
    arrays, first = [], None
    for f in data_files:
        a, pr = read_nifti(f)
        arrays.append(a[None])
        first = first or pr
    properties["original_size_of_raw_data"] = np.array(arrays[0].shape[1:])
    properties["original_spacing"] = np.array(first["itk_spacing"])[[2, 1, 0]]
    properties["list_of_data_files"] = data_files
    properties["seg_file"] = seg_file
    properties["volume_per_voxel"] = float(np.prod(first["itk_spacing"], dtype=np.float64))
    properties["itk_origin"] = first["itk_origin"]
    properties["itk_spacing"] = first["itk_spacing"]
    properties["itk_direction"] = first["itk_direction"]
    if info_dict is not None:
        properties.update(info_dict)
    data_npy = np.vstack(arrays)
    seg_npy = read_nifti(seg_file)[0][None].astype(np.float32) if seg_file is not None else None
    return data_npy.astype(np.float32), seg_npy, properties


def get_case_identifier(case):
    """cropping.py:65-68: `<patient>_<frame>` of a case's first image file `<patient>_<frame>_0000.nii.gz`"""
    return os.path.basename(case[0]).split(".nii.gz")[0][:-5]


def get_case_identifier_from_npz(case):
    return os.path.basename(case)[:-4]


def _save_case(folder, case_identifier, all_data, properties, compress="zlib"):
    """compress="device": all_data is a deflate.Member whose bytes the device loop has already compressed (the writer thread only puts the
    zip container around them), or an array / device tensor that is compressed now."""
    if compress == "zlib":
        np.savez_compressed(os.path.join(folder, "%s.npz" % case_identifier), data=all_data)
    else:
        from . import deflate
        deflate.check_compress(compress)
        member = all_data if isinstance(all_data, deflate.Member) else deflate.npy_member(all_data)
        deflate.write_npz(os.path.join(folder, "%s.npz" % case_identifier), {"data": member})
    with open(os.path.join(folder, "%s.pkl" % case_identifier), "wb") as f:
        pickle.dump(properties, f)


class ImageCropper(object):
    """cropping.py:145-335: the test-time entry points (static) and the training-side driver of the fork, which crops the cases of a
    patient together.  Files are read and compressed by at most 16 threads around the device work; no process pool."""

    def __init__(self, num_threads, output_folder=None, compress="zlib"):
        from .deflate import check_compress
        self.output_folder = output_folder
        self.compress = check_compress(compress)          # "device": the cropped cases are deflated on the device, only the compressed bytes come back
        self.num_threads = max(1, min(16, int(num_threads)))
        self.seconds = {"read": 0.0, "device": 0.0, "write": 0.0}      # where run_cropping spent its time (write: summed over the threads)
        if self.output_folder is not None:
            os.makedirs(self.output_folder, exist_ok=True)

    get_case_identifier = staticmethod(get_case_identifier)

    def _crop_patient(self, loaded):
        """loaded: [(data, seg, properties)] of one patient's cases as numpy.  Every case is uploaded once, cropped to its own non-zero
        box on the device and zero-padded to the union of the patient's boxes -> [(device data, device seg, properties)], the union box."""
        cropped = [ImageCropper.crop(_to_dev(d), p, _to_dev(s)) for d, s, p in loaded]
        boxes = np.stack([np.stack([np.array(b) for b in p["crop_bbox"]]) for _, _, p in cropped])       # [cases, 3, 2]
        lo, hi = np.min(boxes[:, :, 0], axis=0), np.max(boxes[:, :, 1], axis=0)
        union = [list(x) for x in np.stack([lo, hi], axis=-1)]
        return cropped, boxes[:, :, 0] - lo[None], tuple(int(v) for v in hi - lo), union

    def load_crop_save(self, case, case_identifier, overwrite_existing=False, info_dict=None, loaded=None, pool=None):
        """cropping.py:179-236.  case: the patient's cases [[image files ..., label file], ...]; case_identifier / info_dict: one per case.
        loaded: the cases already read (run_cropping reads ahead); pool: an executor for the compressed writes (their futures are returned)."""
        import time
        if loaded is None:
            loaded = [load_case_from_list_of_files(c[:-1], c[-1], None if info_dict is None else info_dict[i]) for i, c in enumerate(case)]
        t0 = time.perf_counter()
        cropped, before, union_size, union = self._crop_patient(loaded)
        writes = []
        for i, (d, s, props) in enumerate(cropped):
            if "Quorum" not in case[i][0]:
                # np.pad of data and seg to the union box: zeros around the case's own box
                full = torch.zeros((d.shape[0] + s.shape[0],) + union_size, dtype=torch.float32, device=d.device)
                sl = (slice(None),) + tuple(slice(int(b), int(b) + n) for b, n in zip(before[i], d.shape[1:]))
                full[:d.shape[0]][sl] = d
                full[d.shape[0]:][sl] = s.float()
            else:
                full = torch.cat([d, s.float()], 0)
            props["size_after_cropping"] = tuple(full.shape[1:])
            props["crop_bbox"] = union
            npz = os.path.join(self.output_folder, "%s.npz" % case_identifier[i])
            if overwrite_existing or not os.path.isfile(npz) or not os.path.isfile(npz[:-4] + ".pkl"):
                if self.compress == "zlib":
                    args = (self.output_folder, case_identifier[i], full.cpu().numpy(), props)
                else:
                    from .deflate import npy_member
                    args = (self.output_folder, case_identifier[i], npy_member(full), props, self.compress)
                if pool is not None:
                    writes.append(pool.submit(self._timed_save, *args))
                else:
                    self.seconds["write"] += self._timed_save(*args)
        self.seconds["device"] += time.perf_counter() - t0
        return writes

    def _timed_save(self, *args):
        import time
        t0 = time.perf_counter()
        _save_case(*args)
        return time.perf_counter() - t0

    def run_cropping(self, list_of_files, overwrite_existing=False, output_folder=None, info_list=None):
        """cropping.py:298-334.  list_of_files: patients -> cases -> [image files ..., label file]; info_list: patients -> cases -> the
        case's dataset.json training entry.  The label files are copied to <output_folder>/gt_segmentations."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from .folder_io import read_ahead
        if output_folder is not None:
            self.output_folder = output_folder
        output_folder_gt = os.path.join(self.output_folder, "gt_segmentations")
        os.makedirs(output_folder_gt, exist_ok=True)
        if info_list is None:
            info_list = [[None] * len(p) for p in list_of_files]
        jobs = []
        for p, patient_info in zip(list_of_files, info_list):
            for case in p:
                if case[-1] is not None:
                    shutil.copy(case[-1], output_folder_gt)
            jobs.append([(case, info) for case, info in zip(p, patient_info)])
        writes = []
        with ThreadPoolExecutor(self.num_threads) as pool:
            t0 = time.perf_counter()
            # (half the threads read ahead -- a patient is a few files -- while the others compress what the device has finished)
            for job, loaded in read_ahead(jobs, lambda ci: load_case_from_list_of_files(ci[0][:-1], ci[0][-1], ci[1]), depth=max(2, self.num_threads // 4),
                                          pool=pool):
                self.seconds["read"] += time.perf_counter() - t0           # what the device waited for, not the threads' total
                p, info = [c for c, _ in job], [i for _, i in job]
                writes += self.load_crop_save(p, [get_case_identifier(c) for c in p], overwrite_existing, info, loaded=loaded, pool=pool)
                t0 = time.perf_counter()
            self.seconds["write"] += sum(w.result() for w in writes)

    @staticmethod
    def crop(data, properties, seg=None):
        data, seg, bbox = crop_to_nonzero(data, seg, nonzero_label=-1)
        properties["crop_bbox"] = bbox
        properties["classes"] = torch.unique(seg).cpu().numpy() if torch.is_tensor(seg) else np.unique(seg)
        seg[seg < -1] = 0
        properties["size_after_cropping"] = tuple(data[0].shape)
        return data, seg, properties

    @staticmethod
    def crop_from_list_of_files(data_files, seg_file=None, info_dict=None):
        data, seg, properties = load_case_from_list_of_files(data_files, seg_file, info_dict)
        return ImageCropper.crop(data, properties, seg)


# ------------------------------------------------------------------------------------------------ preprocessing.py
def get_do_separate_z(spacing, anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """preprocessing.py:30-32."""
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(new_spacing):
    """preprocessing.py:35-37."""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def _spline_axis(x, axis, m):
    """one cubic-spline pass: x fp64 device tensor, `axis` resampled to m samples"""
    if x.shape[axis] == m:
        return x
    x = x.contiguous()
    n = x.shape[axis]
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    out = torch.empty(x.shape[:axis] + (m,) + x.shape[axis + 1:], dtype=torch.float64, device=x.device)
    check(lib().cf_spline3_resample_axis(x.data_ptr(), out.data_ptr(), outer, n, inner, m, _stream()), "cf_spline3_resample_axis")
    return out


def _resize_cubic(t, new_shape, slab_axis):
    """skimage resize(order=3, mode='edge', clip=True, anti_aliasing=False) of every channel of t [C, x, y, z] (fp32 device):
    per 2-D slice along `slab_axis` (1..3, that axis keeps its size) or of the whole 3-D channel (slab_axis None)."""
    C = t.shape[0]
    x = t.double()
    dims = list(x.shape)
    if slab_axis is None:
        A, S, B = 1, 1, int(np.prod(dims[1:], dtype=np.int64))
    else:
        A, S, B = int(np.prod(dims[1:slab_axis], dtype=np.int64)), dims[slab_axis], int(np.prod(dims[slab_axis + 1:], dtype=np.int64))
    mm = torch.empty(C * S * 2, dtype=torch.float64, device=x.device)
    part = torch.empty(C * S * 2 * lib().cf_slab_minmax_chunks(C, A, S, B), dtype=torch.float64, device=x.device)
    check(lib().cf_slab_minmax(x.data_ptr(), C, A, S, B, mm.data_ptr(), part.data_ptr(), _stream()), "cf_slab_minmax")
    for a in (1, 2, 3):
        if a != slab_axis:
            x = _spline_axis(x, a, int(new_shape[a - 1]))
    dims = list(x.shape)
    if slab_axis is None:
        A, S, B = 1, 1, int(np.prod(dims[1:], dtype=np.int64))
    else:
        A, S, B = int(np.prod(dims[1:slab_axis], dtype=np.int64)), dims[slab_axis], int(np.prod(dims[slab_axis + 1:], dtype=np.int64))
    out = torch.empty(dims, dtype=torch.float32, device=x.device)
    check(lib().cf_slab_clip_to_f32(x.contiguous().data_ptr(), _f32(out), C, A, S, B, mm.data_ptr(), _stream()), "cf_slab_clip_to_f32")
    return out


def _resize_labels(t, new_shape, lin):
    """batchgenerators' resize_segmentation for order 1: every label's indicator is resized (linear on the axes flagged in `lin`,
    nearest on the others) and the label assigned where it reaches 0.5, labels ascending.  t [C, x, y, z] fp32 on the device.
    One kernel (ops.resize_labels): the reference's fp64 indicator chain, so indicators of exactly 0.5 fall on its side."""
    return ops.resize_labels(t, new_shape, lin)


def resize_segmentation(segmentation, new_shape, order=1):
    """batchgenerators.augmentations.utils.resize_segmentation on the device route of `resample_data_or_seg`: order 0 resizes the label
    map itself (nearest), order 1 resizes every label's indicator and assigns the label where it reaches 0.5, labels ascending.
    segmentation: 2-D or 3-D, numpy or device tensor; the same kind and dtype come back.  Other orders are not built."""
    was_numpy = not torch.is_tensor(segmentation)
    assert len(segmentation.shape) == len(new_shape), "new shape must have same dimensionality as segmentation"
    if order not in (0, 1):
        raise NotImplementedError("resize_segmentation is built for orders 0 and 1 (got %s)" % (order,))
    t = torch.from_numpy(np.ascontiguousarray(segmentation)) if was_numpy else segmentation
    if t.dim() not in (2, 3):
        raise ValueError("resize_segmentation takes a 2-D or 3-D label map, got shape %s" % (tuple(t.shape),))
    dtype_in = t.dtype
    lead = (1,) * (3 - t.dim())
    new3 = lead + tuple(int(v) for v in new_shape)                          # (a 2-D map is a one-slice volume: that axis keeps its sample)
    t = t.to(_dev(), dtype=torch.float32).reshape((1,) + lead + tuple(t.shape)).contiguous()
    out = ops.resize3d(t, new3, [0, 0, 0]).round() if order == 0 else _resize_labels(t, new3, [1, 1, 1])
    out = out.reshape(new3[len(lead):]).to(dtype_in)
    return out.cpu().numpy() if was_numpy else out


def to_one_hot(seg, all_seg_labels=None):
    """nnunet/utilities/one_hot_encoding.py: [len(labels), *seg.shape] of seg's dtype, plane i is 1 where seg == all_seg_labels[i]
    (default: the labels present).  numpy or tensor in, the same kind out."""
    if torch.is_tensor(seg):
        labels = torch.unique(seg).tolist() if all_seg_labels is None else list(all_seg_labels)
        return torch.stack([(seg == l_) for l_ in labels]).to(seg.dtype) if labels else seg.new_zeros((0,) + tuple(seg.shape))
    labels = np.unique(seg) if all_seg_labels is None else all_seg_labels
    result = np.zeros((len(labels),) + tuple(seg.shape), dtype=seg.dtype)
    for i, l_ in enumerate(labels):
        result[i][seg == l_] = 1
    return result


def prev_stage_to_input(data, seg_prev, classes):
    """nnunet/inference/predict.py:82-85 -- the network input of a cascade's full-resolution stage: `data` [C, X2, Y2, Z2] (preprocessed,
    float32) with the previous stage's label map `seg_prev` [X, Y, Z] (already transposed, labels 0..255) appended as len(classes)
    one-hot channels on data's grid.  One kernel (ops.prev_stage_onehot) resizes and encodes the labels straight into channels C.. of
    the result: no intermediate label volume, no per-label pass, no vstack.  numpy or device tensor in (data decides), same kind out."""
    was_numpy = not torch.is_tensor(data)
    d = _to_dev(data)
    assert d.dim() == 4 and len(seg_prev.shape) == 3, "data must be (c, x, y, z) and seg_prev (x, y, z)"
    classes = [int(c) for c in classes]
    s = seg_prev if torch.is_tensor(seg_prev) else torch.from_numpy(np.ascontiguousarray(seg_prev))
    if s.dtype != torch.uint8:
        lo, hi = (int(v) for v in torch.aminmax(s))
        if lo < 0 or hi > 255:
            raise ValueError("prev_stage_to_input: previous-stage labels must lie in 0..255, got %d..%d" % (lo, hi))
    s = s.to(d.device, dtype=torch.uint8).contiguous()
    C = d.shape[0]
    out = torch.empty((C + len(classes),) + tuple(d.shape[1:]), dtype=torch.float32, device=d.device)
    out[:C].copy_(d)
    ops.prev_stage_onehot(s, classes, out[C:])
    return out.cpu().numpy() if was_numpy else out


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, order_z=0):
    """preprocessing.py:111-200.  data (c, x, y, z), numpy or device tensor (the same kind is returned).  Built: data of order
    0, 1 or 3 and segmentations of order 0 or 1, with order_z 0 or 1 (data) / 0 (segmentations) along the separate axis."""
    was_numpy = not torch.is_tensor(data)
    t = torch.from_numpy(np.ascontiguousarray(data)) if was_numpy else data
    dtype_in = t.dtype
    assert t.dim() == 4 and len(new_shape) == 3, "data must be (c, x, y, z)"
    new_shape = tuple(int(v) for v in new_shape)
    if tuple(t.shape[1:]) == new_shape:
        return data
    if order not in (0, 1, 3) or order_z not in (0, 1):
        raise NotImplementedError("resampling is built for interpolation orders 0, 1 and 3 in-plane and 0 / 1 along z (got %s / %s)" % (order, order_z))
    if is_seg and (order not in (0, 1) or (do_separate_z and order_z != 0)):
        raise NotImplementedError("segmentation resampling is built for orders 0 and 1 (order_z 0)")
    t = t.to(_dev(), dtype=torch.float32).contiguous()
    sep = None
    if do_separate_z:
        assert len(axis) == 1, "only one anisotropic axis supported"
        sep = int(axis[0])
    lin = [int(order != 0)] * 3
    if sep is not None:
        lin[sep] = int(order_z)
    if is_seg:
        out = ops.resize3d(t, new_shape, [0, 0, 0]) if order == 0 else _resize_labels(t, new_shape, lin)
    elif order == 3:
        if sep is None:
            out = _resize_cubic(t, new_shape, None)
        else:
            inplane = list(new_shape)
            inplane[sep] = t.shape[1 + sep]
            out = _resize_cubic(t, inplane, 1 + sep)            # every slice on its own, clipped to its own range, cast to fp32
            if t.shape[1 + sep] != new_shape[sep]:
                zl = [0, 0, 0]
                zl[sep] = int(order_z)
                out = ops.resize3d(out, new_shape, zl)          # the map_coordinates pass along the separate axis
    else:
        out = ops.resize3d(t, new_shape, lin)
    if is_seg and order == 0:
        out = out.round()
    out = out.to(dtype_in)
    return out.cpu().numpy() if was_numpy else out


def resample_patient(data, seg, original_spacing, target_spacing, order_data=3, order_seg=0, force_separate_z=False, order_z_data=0,
                     order_z_seg=0, separate_z_anisotropy_threshold=RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD):
    """preprocessing.py:40-108."""
    assert not ((data is None) and (seg is None))
    if data is not None:
        assert len(data.shape) == 4, "data must be c x y z"
    if seg is not None:
        assert len(seg.shape) == 4, "seg must be c x y z"
    shape = np.array(data[0].shape if data is not None else seg[0].shape)
    new_shape = np.round(((np.array(original_spacing) / np.array(target_spacing)).astype(float) * shape)).astype(int)
    if force_separate_z is not None:
        do_separate_z = force_separate_z
        axis = get_lowres_axis(original_spacing) if force_separate_z else None
    elif get_do_separate_z(original_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(original_spacing)
    elif get_do_separate_z(target_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(target_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) != 1:
        do_separate_z = False       # (0.24, 1.25, 1.25)-like spacings: no separate out-of-plane pass
    data_reshaped = resample_data_or_seg(data, new_shape, False, axis, order_data, do_separate_z, order_z=order_z_data) if data is not None else None
    seg_reshaped = resample_data_or_seg(seg, new_shape, True, axis, order_seg, do_separate_z, order_z=order_z_seg) if seg is not None else None
    return data_reshaped, seg_reshaped


def _moments(x, seg, lo=None, hi=None):
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    use_range = lo is not None
    check(lib().cf_masked_moments(_f32(x), None if seg is None else _f32(seg), x.numel(), int(use_range), float(lo or 0.0), float(hi or 0.0),
                                  out.data_ptr(), _stream()), "cf_masked_moments")
    s1, s2, n = out.cpu().tolist()
    if n == 0:
        return float("nan"), float("nan")
    mean = s1 / n
    return mean, float(np.sqrt(max(s2 / n - mean * mean, 0.0)))


def _normalize(x, seg, sub, div, clip=None, zero_outside=False):
    lo, hi = clip if clip is not None else (0.0, 0.0)
    check(lib().cf_normalize(_f32(x), None if seg is None else _f32(seg), x.numel(), int(clip is not None), float(lo), float(hi), float(sub), float(div),
                             int(zero_outside), _stream()), "cf_normalize")


class GenericPreprocessor(object):
    """preprocessing.py:202-331 (test-time methods)."""

    resample_order_seg_test = 1
    compress = "zlib"          # "device": run() deflates the stage folders' .npz on the device (an attribute, so that planners need no new argument)

    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties=None):
        self.transpose_forward = transpose_forward
        self.intensityproperties = intensityproperties
        self.normalization_scheme_per_modality = normalization_scheme_per_modality
        self.use_nonzero_mask = use_nonzero_mask
        self.resample_separate_z_anisotropy_threshold = RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD
        self.resample_order_data = 3
        self.resample_order_seg = 1

    def _target_spacing(self, target_spacing, original_spacing_transposed):
        return np.array(target_spacing, dtype=float)

    def resample_and_normalize(self, data, target_spacing, properties, seg=None, force_separate_z=None):
        """preprocessing.py:233-321.  data / seg already transposed by transpose_forward; properties are the un-transposed values."""
        was_numpy = not torch.is_tensor(data)
        original_spacing_transposed = np.array(properties["original_spacing"])[list(self.transpose_forward)]
        target_spacing = self._target_spacing(target_spacing, original_spacing_transposed)
        seg_dtype = None if seg is None else seg.dtype
        d = _to_dev(data)
        if self._remove_nans:
            d = d.clone() if d.data_ptr() == (data.data_ptr() if torch.is_tensor(data) else 0) else d
            check(lib().cf_nan_to_zero(_f32(d), d.numel(), _stream()), "cf_nan_to_zero")
        s = None if seg is None else _to_dev(seg)
        d, s = resample_patient(d, s, np.array(original_spacing_transposed), target_spacing, self.resample_order_data, self.resample_order_seg,
                                force_separate_z=force_separate_z, order_z_data=0, order_z_seg=0,
                                separate_z_anisotropy_threshold=self.resample_separate_z_anisotropy_threshold)
        d = d.contiguous()
        if s is not None:
            s = s.contiguous()
            s[s < -1] = 0
        properties["size_after_resampling"] = tuple(d[0].shape)
        properties["spacing_after_resampling"] = target_spacing
        assert len(self.normalization_scheme_per_modality) == len(d), "self.normalization_scheme_per_modality must have as many entries as data has modalities"
        assert len(self.use_nonzero_mask) == len(d), "self.use_nonzero_mask must have as many entries as data has modalities"
        for c in range(len(d)):
            scheme = self.normalization_scheme_per_modality[c]
            masked = bool(self.use_nonzero_mask[c])
            if scheme in ("CT", "CT2"):
                assert self.intensityproperties is not None, "ERROR: if there is a CT then we need intensity properties"
                ip = self.intensityproperties[c]
                lb, ub = ip["percentile_00_5"], ip["percentile_99_5"]
                if scheme == "CT":
                    mn, sd = ip["mean"], ip["sd"]
                else:
                    mn, sd = _moments(d[c], None, lb, ub)
                _normalize(d[c], s[-1] if masked else None, mn, sd, clip=(lb, ub), zero_outside=masked)
            elif scheme == "noNorm":
                pass
            else:
                mn, sd = _moments(d[c], s[-1] if masked else None)
                _normalize(d[c], s[-1] if masked else None, np.float32(mn), np.float32(sd) + np.float32(1e-8), zero_outside=masked)
        if was_numpy:
            return d.cpu().numpy(), None if s is None else s.cpu().numpy().astype(seg_dtype), properties
        return d, None if s is None else s.to(seg_dtype), properties

    _remove_nans = True

    def preprocess_test_case(self, data_files, target_spacing=None, seg_file=None, force_separate_z=None, need_seg=True, seg_from_prev_stage=None,
                             prev_stage_classes=None):
        """preprocessing.py:323-331 -> (data float32 [C, ...], seg, properties), numpy like the reference.  The case goes to the device once
        and comes back once: crop, transpose, resampling and normalisation hand device tensors to each other (the numpy-in / numpy-out
        functions above cost two more 2 MB copies and a 4 MB int64 label map per frame, with a stream synchronisation each, which the
        file-level API paid under a running network batch -- profiles/r03_api_split.md).  need_seg=False skips the label map's read-back.
        seg_from_prev_stage (a .nii.gz label file of the cascade's previous stage) + prev_stage_classes: nnunet/inference/predict.py:68-85 --
        the UNCROPPED label map, transposed, is resized onto the cropped and resampled grid and appended as one-hot channels
        (prev_stage_to_input), before the case leaves the device."""
        data, seg, properties = load_case_from_list_of_files(data_files, seg_file)
        seg_prev = None
        if seg_from_prev_stage is not None:
            assert os.path.isfile(seg_from_prev_stage) and seg_from_prev_stage.endswith(".nii.gz"), \
                "segs_from_prev_stage must point to a segmentation file"
            seg_prev = read_nifti(seg_from_prev_stage)[0]
            assert all([i == j for i, j in zip(seg_prev.shape, data.shape[1:])]) and seg_prev.ndim == data.ndim - 1, \
                "image and segmentation from previous stage don't have the same pixel array shape! image: %s, seg_prev: %s" % \
                (data_files[0], seg_from_prev_stage)
            seg_prev = seg_prev.transpose(self.transpose_forward)
        data, seg, properties = ImageCropper.crop(_to_dev(data), properties, None if seg is None else _to_dev(seg))
        tf = (0, *[i + 1 for i in self.transpose_forward])
        if target_spacing is None:        # (plans without stages: the case keeps its own spacing)
            target_spacing = np.array(properties["original_spacing"], dtype=float)[list(self.transpose_forward)]
        d, s, properties = self.resample_and_normalize(data.permute(tf).contiguous(), target_spacing, properties, seg.permute(tf).contiguous(),
                                                       force_separate_z=force_separate_z)
        if seg_prev is not None:
            d = prev_stage_to_input(d, seg_prev, prev_stage_classes)
        return d.cpu().numpy().astype(np.float32, copy=False), (s.cpu().numpy() if need_seg else None), properties

    @staticmethod
    def load_cropped(cropped_output_dir, case_identifier):
        """preprocessing.py:219-226 -> (all_data [C + 1, X, Y, Z] as stored, properties)"""
        from .safe_pickle import load_plain_pickle
        all_data = np.load(os.path.join(cropped_output_dir, "%s.npz" % case_identifier))["data"]
        return all_data, load_plain_pickle(os.path.join(cropped_output_dir, "%s.pkl" % case_identifier))

    @staticmethod
    def class_locations(seg, all_classes, num_samples=10000, min_percent_coverage=0.01, seed=1234):
        """preprocessing.py:403-421 for a device label volume [X, Y, Z] (float32): per foreground class up to num_samples voxel
        coordinates (at least min_percent_coverage of the class), drawn without replacement by ONE np.random.RandomState(seed) that the
        classes consume in all_classes order -- np.argwhere(seg == c)[rndst.choice(n, target, replace=False)] without the argwhere: the
        counts come from the count pass, the coordinates from the select kernel.  -> {class: int64 [target, 3] or []}"""
        rndst = np.random.RandomState(seed)
        class_locs = {}
        seg = seg.contiguous()
        for g in range(0, len(all_classes), 16):                    # (a count pass takes 16 values)
            group = list(all_classes[g:g + 16])
            index = ops.RankIndex(seg, group)
            for c, n in zip(group, index.totals.tolist()):
                if n == 0:
                    class_locs[c] = []
                    continue
                target = max(min(num_samples, n), int(np.ceil(n * min_percent_coverage)))
                class_locs[c] = ops.select_coords(seg, c, rndst.choice(n, target, replace=False), index).cpu().numpy()
        return class_locs

    def _run_case(self, all_data, properties, target_spacings, force_separate_z, all_classes, keep_spacing, compress="zlib"):
        """preprocessing.py:387-427 for every stage of one labelled case: all_data [C + 1, X, Y, Z] (numpy, the cropped .npz) goes to the
        device once -> [(all_data float32 numpy, properties)] per stage; compress="device": the stage's array as a deflate.Member, compressed
        and checksummed before it leaves the device"""
        tf = (0, *[i + 1 for i in self.transpose_forward])
        t = _to_dev(all_data).permute(tf).contiguous()
        out = []
        for target_spacing in target_spacings:
            props = copy.deepcopy(properties)
            if keep_spacing:
                target_spacing = props["original_spacing"]
            d, s, props = self.resample_and_normalize(t[:-1].clone(), target_spacing, props, t[-1:].clone(), force_separate_z)   # (normalised in place)
            staged = torch.cat([d, s.float()], 0)
            props["class_locations"] = self.class_locations(staged[-1], all_classes)
            if compress == "zlib":
                out.append((staged.cpu().numpy(), props))
            else:
                from .deflate import npy_member
                out.append((npy_member(staged), props))
        return out

    def run(self, target_spacings, input_folder_with_cropped_npz, output_folder, data_identifier, num_threads=8, force_separate_z=None,
            keep_spacing=False, compress=None):
        """preprocessing.py:429-467 / :704-730, labelled cases: <output_folder>/<data_identifier>_stage<k>/<case>.npz + .pkl for every
        cropped case and stage.  Case-major: a case is read once (ahead, by the thread pool), uploaded once and leaves the device once
        per stage; the compressed writes run on the same pool of at most 16 threads."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from .folder_io import read_ahead, subfiles
        from .safe_pickle import load_plain_pickle
        cases = [get_case_identifier_from_npz(c) for c in subfiles(input_folder_with_cropped_npz, suffix=".npz")]
        assert len(cases) != 0, "set list of files first"
        os.makedirs(output_folder, exist_ok=True)
        all_classes = load_plain_pickle(os.path.join(input_folder_with_cropped_npz, "dataset_properties.pkl"))["all_classes"]
        stage_folders = [os.path.join(output_folder, data_identifier + "_stage%d" % i) for i in range(len(target_spacings))]
        for f in stage_folders:
            os.makedirs(f, exist_ok=True)
        self.seconds = {"read": 0.0, "device": 0.0, "write": 0.0}
        threads = max(1, min(16, int(num_threads[-1] if isinstance(num_threads, (list, tuple, np.ndarray)) else num_threads)))

        from .deflate import check_compress
        compress = check_compress(compress or self.compress)

        def save(folder, case, arr, props):
            t0 = time.perf_counter()
            _save_case(folder, case, arr, props, compress)
            return time.perf_counter() - t0

        writes = []
        with ThreadPoolExecutor(threads) as pool:
            t0 = time.perf_counter()
            for (case,), (loaded,) in read_ahead([[c] for c in cases], lambda c: self.load_cropped(input_folder_with_cropped_npz, c), depth=max(2, threads // 2),
                                                   pool=pool):
                t1 = time.perf_counter()
                self.seconds["read"] += t1 - t0
                if "_u" in case:
                    raise NotImplementedError("%s: unlabeled cases (`_u`) are not built" % case)
                for folder, (arr, props) in zip(stage_folders, self._run_case(loaded[0], loaded[1], target_spacings, force_separate_z, all_classes,
                                                                             keep_spacing, compress)):
                    writes.append(pool.submit(save, folder, case, arr, props))
                t0 = time.perf_counter()
                self.seconds["device"] += t0 - t1
            self.seconds["write"] += sum(w.result() for w in writes)

    def preprocess_arrays(self, data, seg, properties, target_spacing, force_separate_z=None):
        tf = (0, *[i + 1 for i in self.transpose_forward])
        data = data.transpose(tf)
        seg = seg.transpose(tf)
        data, seg, properties = self.resample_and_normalize(data, target_spacing, properties, seg, force_separate_z=force_separate_z)
        return data.astype(np.float32), seg, properties


class PreprocessorFor2D(GenericPreprocessor):
    """preprocessing.py:699-803: the first (slice) axis keeps its spacing; NaNs are not touched."""

    _remove_nans = False

    def _target_spacing(self, target_spacing, original_spacing_transposed):
        ts = np.array(target_spacing, dtype=float)
        ts[0] = original_spacing_transposed[0]
        return ts
