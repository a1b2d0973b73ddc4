"""nnUNet_ensemble_predictions on the HIP path: average the saved softmax of several prediction folders.

Mirrors `nnunet/inference/ensemble_predictions.py` (public names, argument lists and defaults of `merge_files` :26, `merge` :56 and the CLI
flags of `main` :98-124).  Its inputs are the `<case>.npz` (`softmax`, [K,Z,Y,X]) + `<case>.pkl` (properties) pairs that
`predict_from_folder(..., save_npz=True)` writes, of this project or of the reference; its outputs are `<case>.nii.gz` uint8 label files
with the case's geometry, `<case>.npz` / `.pkl` with `--npz`, and the postprocessed files when a `postprocessing.json` is given.

The mean over the folders, the arg-max (or the `regions_class_order` overwrite loop of segmentation_export.py:147-151) and the placement
into the volume before cropping (:153-162) are one kernel, `cineflow.ops.ensemble_merge`; its numbers are those of the reference's
`np.mean(np.vstack(softmax), 0)` bit for bit.  Files are read and inflated by a pool of `threads` workers, the next case's while the device
and the writers work on this one.

Differences that are deliberate:
  * a case is an `.npz` path relative to its folder, looked for in the folder itself (the reference's flat layout) and one level of
    sub-folders down (`<out>/<patient>/<case>.npz`, what this project's segmentation-only route writes); the output keeps the relative path;
  * property files go through `cineflow.safe_pickle` (plain containers and numpy values only), never through `pickle.load`;
  * members whose softmax shapes differ, a softmax that is not of the properties' `size_after_cropping` (nothing is resampled here, as in
    the reference) and a crop that overhangs the volume are refused with a ValueError that names the case, before any device work;
  * `threads` is a thread pool, not a process pool: one process holds the device.
`LAST_TIMING` holds the load / device / write seconds of the last `merge_files` call."""
import argparse
import os
import pickle
import shutil
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .folder_io import load_softmax as _load_softmax, read_ahead, softmax_case_geometry   # (the private name: the one its tests patch)
from .nifti import write_nifti
from .safe_pickle import load_plain_pickle

join = os.path.join
isfile = os.path.isfile

LAST_TIMING = {}


def find_cases(folders):
    """Sorted union over the folders of the `.npz` files of each folder and of its direct sub-folders, as paths relative to the folder and
    without the extension."""
    cases = set()
    for folder in folders:
        for name in os.listdir(folder):
            path = join(folder, name)
            if isfile(path):
                if name.endswith(".npz"):
                    cases.add(name[:-4])
            elif os.path.isdir(path):
                cases.update(join(name, n[:-4]) for n in os.listdir(path) if n.endswith(".npz") and isfile(join(path, n)))
    return sorted(cases)


def _regions_class_order(props, files):
    """ensemble_predictions.py:33-45."""
    reg_class_orders = [p["regions_class_order"] if "regions_class_order" in p.keys() else None for p in props]
    if all(i is None for i in reg_class_orders):
        return None
    tmp = reg_class_orders[0]
    for r in reg_class_orders[1:]:
        assert tmp == r, "If merging files with regions_class_order, the regions_class_orders of all " \
                         "files must be the same. regions_class_order: %s, \n files: %s" % (str(reg_class_orders), str(files))
    return tmp


def _check_case(softmax, props, files):
    """Everything that can be refused on the host -> (full_shape, bbox_lo, regions_class_order) for ops.ensemble_merge."""
    regions_class_order = _regions_class_order(props, files)
    shapes = [tuple(s.shape) for s in softmax]
    if any(len(s) != 4 for s in shapes) or any(s != shapes[0] for s in shapes):
        raise ValueError("%s: the members' softmax shapes differ or are not [K,Z,Y,X]: %s" % (files[0], shapes))
    dtypes = [s.dtype for s in softmax]
    if dtypes[0] not in (np.float16, np.float32) or any(d != dtypes[0] for d in dtypes):
        raise ValueError("%s: the members' softmax must be all float16 or all float32, got %s" % (files[0], [str(d) for d in dtypes]))
    full, lo = softmax_case_geometry(shapes[0], props[0], files[0])
    if regions_class_order is not None and len(regions_class_order) != shapes[0][0]:
        raise ValueError("%s: regions_class_order %s does not name the %d channels of the softmax" % (files[0], regions_class_order, shapes[0][0]))
    return full, lo, regions_class_order


def _merge_loaded(softmax, props, files, store_npz):
    """-> (labels uint8 [Zf,Yf,Xf], mean or None) as numpy, through one ops.ensemble_merge"""
    full, lo, regions_class_order = _check_case(softmax, props, files)
    import torch
    from . import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    members = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in softmax]
    seg, mean = ops.ensemble_merge(members, full, lo, want_mean=bool(store_npz), regions_class_order=regions_class_order)
    return seg.cpu().numpy(), (mean.cpu().numpy() if mean is not None else None)


def _write_labels(seg, props, out_file):
    first = props[0]
    write_nifti(out_file, seg, first["itk_spacing"], first["itk_origin"], first["itk_direction"])


# who deflates the mean softmax's .npz: "zlib" (np.savez_compressed), or "device" (cineflow.deflate).  merge and merge_files keep the
# reference's argument lists, so the choice is this module attribute; _write_npz itself takes it as a keyword.
NPZ_COMPRESS = "zlib"


def _write_npz(mean, props, out_file, compress="zlib"):
    if compress == "zlib":
        np.savez_compressed(out_file[:-7] + ".npz", softmax=mean)
    else:
        from . import deflate
        deflate.check_compress(compress)
        deflate.savez_compressed(out_file[:-7] + ".npz", softmax=mean)
    with open(out_file[:-7] + ".pkl", "wb") as f:
        pickle.dump(props, f)


def merge_files(files, properties_files, out_file, override, store_npz):
    """ensemble_predictions.py:26-53 for one case."""
    if not (override or not isfile(out_file)):
        return
    t0 = time.perf_counter()
    softmax = [_load_softmax(f) for f in files]
    props = [load_plain_pickle(f) for f in properties_files]
    t1 = time.perf_counter()
    seg, mean = _merge_loaded(softmax, props, files, store_npz)
    t2 = time.perf_counter()
    _write_labels(seg, props, out_file)
    if store_npz:
        _write_npz(mean, props, out_file, NPZ_COMPRESS)
    t3 = time.perf_counter()
    LAST_TIMING.clear()
    LAST_TIMING.update(load_s=t1 - t0, device_s=t2 - t1, write_s=t3 - t2)


def merge(folders, output_folder, threads, override=True, postprocessing_file=None, store_npz=False):
    """ensemble_predictions.py:56-95."""
    os.makedirs(output_folder, exist_ok=True)
    if postprocessing_file is not None:
        output_folder_orig = output_folder
        output_folder = join(output_folder, "not_postprocessed")
        os.makedirs(output_folder, exist_ok=True)
    else:
        output_folder_orig = None

    patient_ids = find_cases(folders)
    for f in folders:
        assert all([isfile(join(f, i + ".npz")) for i in patient_ids]), "Not all patient npz are available in " \
                                                                        "all folders"
        assert all([isfile(join(f, i + ".pkl")) for i in patient_ids]), "Not all patient pkl are available in " \
                                                                        "all folders"
    files, property_files, out_files = [], [], []
    for p in patient_ids:
        out_file = join(output_folder, p + ".nii.gz")
        if override or not isfile(out_file):
            files.append([join(f, p + ".npz") for f in folders])
            property_files.append([join(f, p + ".pkl") for f in folders])
            out_files.append(out_file)

    with ThreadPoolExecutor(max(1, int(threads))) as pool:
        writes = []
        cases = read_ahead(files, _load_softmax, depth=1, pool=pool)     # the next case inflates while the device and the writers work
        for i, (_, softmax) in enumerate(cases):
            out_file = out_files[i]
            props = [load_plain_pickle(f) for f in property_files[i]]
            seg, mean = _merge_loaded(softmax, props, files[i], store_npz)
            os.makedirs(os.path.dirname(out_file), exist_ok=True)
            writes.append(pool.submit(_write_labels, seg, props, out_file))
            if store_npz:
                writes.append(pool.submit(_write_npz, mean, props, out_file, NPZ_COMPRESS))
        for w in writes:
            w.result()

    if postprocessing_file is not None:
        from .export import load_postprocessing, load_remove_save
        for_which_classes, min_valid_obj_size = load_postprocessing(postprocessing_file)
        print("Postprocessing...")
        for p in patient_ids:                                             # apply_postprocessing_to_folder, connected_components.py:402-425
            os.makedirs(os.path.dirname(join(output_folder_orig, p)), exist_ok=True)
            load_remove_save(join(output_folder, p + ".nii.gz"), join(output_folder_orig, p + ".nii.gz"), for_which_classes, min_valid_obj_size)
        shutil.copy(postprocessing_file, output_folder_orig)


def build_parser():
    parser = argparse.ArgumentParser(description="Average the softmax files (<case>.npz + <case>.pkl, written by a prediction with -z / --save_npz) "
                                                 "of several prediction folders and write the label files of the ensemble.")
    parser.add_argument("-f", "--folders", nargs="+", required=True, help="prediction folders to merge; each must hold every case's .npz and .pkl")
    parser.add_argument("-o", "--output_folder", required=True, type=str, help="folder for the merged label files")
    parser.add_argument("-t", "--threads", required=False, default=2, type=int, help="workers that read the .npz files and write the outputs")
    parser.add_argument("-pp", "--postprocessing_file", required=False, type=str, default=None,
                        help="postprocessing.json of the ensemble; without it the merged files are not postprocessed")
    parser.add_argument("--npz", action="store_true", required=False, help="also write the mean softmax (.npz) and the members' properties (.pkl)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    merge(args.folders, args.output_folder, args.threads, override=True, postprocessing_file=args.postprocessing_file, store_npz=args.npz)


if __name__ == "__main__":
    main()
