"""The tables the reference's users read after a cine prediction, from this project's output folders, one device visit per patient.

    python -m cineflow.score seg      -pred FOLDER -ref GT_FOLDER    [-i INPUT_FOLDER] [--gt frame|ed] [--layout predict|saver]
    python -m cineflow.score jacobian -flow FOLDER -l LABEL_FOLDER   [-i INPUT_FOLDER] [--layout predict|saver]
    python -m cineflow.score ssim     -flow FOLDER -i INPUT_FOLDER   [-l LABEL_FOLDER] [--layout predict|saver] [--win 7]
    python -m cineflow.score contour  -flow FOLDER -c CONTOUR_FOLDER -i INPUT_FOLDER [--layout predict|saver]
                                      [--mode from_ed|from_ed_accumulation|to_ed|to_ed_accumulation]

`seg` writes what nnunet/compute_metrics.py writes -- segmentation_metrics.json, segmentation_metrics.csv, segmentation_metrics_es.csv:
Dice, Hausdorff distance and average symmetric surface distance of the propagated labels (RV = 1, MYO = 2, LV = 3) per frame --
and `jacobian` what nnunet/compute_jacobian.py writes -- jacobian.json, jacobian_metrics.csv: the Jacobian statistics and flow
gradients per slice and frame.  `ssim` writes what nnunet/compute_SSIM.py writes -- ssim_metrics.json, ssim_metrics.csv: the structural
similarity of every frame's image INPUT_FOLDER/<patient>/<case>_0000.nii.gz, warped onto the ED frame with the case's flow, to the ED
image, per slice -- and with -l what nnunet/compute_SSIM_crop_per_structure.py writes -- ssim_metrics_all.json, ssim_metrics_all.csv: the
SSIM map's means over the RV, MYO and LV of the ED label volume as well (cineflow.metrics.cine_ssim_table).  All are written from the scripts' behaviour, not transcribed: the scripts' hard-coded paths, pickles
and `patient029` special cases are arguments or gone, and the numbers of a patient come from cineflow.metrics.cine_label_scores /
cine_jacobian_table (csrc/score.hip) instead of one call chain per frame and class.  `contour` writes what
nnunet/compute_contour_metrics.py writes -- contour_metrics.json, contour_metrics.csv: the tracking error of the ground-truth endo-, epi-
and RV contour points CONTOUR_FOLDER/contour/{LV,RV}/<patient>_sliceNN.npy ([4, P, T] and [2, P2, T], 1-based, NN = slice + 1) under the
predicted flow, per slice and frame, in one of the script's four modes (the script picks one from the training config; from_ed is its
fallback and the default here) -- and in mode from_ed also strain_metrics.json: the radial and circumferential strain curves of
nnunet/get_strain.py and their smoothness, with the pixel spacing of the ED image INPUT_FOLDER/<patient>/<case>_0000.nii.gz
(cineflow.strain.track_patient, csrc/contour.hip).

Layouts (one sub-folder per patient either way):
    predict   <FOLDER>/<patient>/Registered/<case>.nii.gz, <FOLDER>/<patient>/Flow/<case>.npz          (cineflow.predict)
    saver     <FOLDER>/Postprocessed/Registered/<patient>/[temp_allClasses/]<case>.nii.gz,
              <FOLDER>/Postprocessed/Flow/<patient>/<case>.npz                                          (cineflow.voxelmorph_saver)
A case's frame number is int(stem[-2:]); cases are sorted by it.  ED / ES indices come from INPUT_FOLDER/<patient>/<patient>.csv
(cineflow.predict.get_ed_es_indices), both 0 without -i; the frame number of index k is k + 1.

A thread pool reads and inflates the next patient's files while the current one is scored; one patient is resident on the device at a
time and only this process opens the GPU.  Turning per-case rows into the json / csv documents is host code (segmentation_tables,
jacobian_tables, ssim_tables, contour_tables, strain_tables).
"""
import collections
import csv
import os
import warnings
import zipfile
import zlib

import numpy as np

from .folder_io import read_ahead, save_json
from .nifti import read_nifti

join = os.path.join

STRUCTURES = ("RV", "MYO", "LV")
SEG_METRICS = ("Dice", "HD", "ASSD")
SEG_COLUMNS = ["Name", "Average_Dice", "Average_HD", "Average_ASSD"] + ["%s_%s" % (s, m) for s in STRUCTURES for m in SEG_METRICS]
READERS = 8

# one file of a patient: `name` the stem, `frame` its number (int(stem[-2:])), `path` the file, `other` its reference / label file
Case = collections.namedtuple("Case", "name frame path other")


# ------------------------------------------------------------------------------------------------ discovery
def frame_number(stem):
    return int(stem[-2:])


def _stem(fname, suffix):
    return os.path.basename(fname)[:-len(suffix)]


def patient_folders(folder, layout, kind):
    """{patient: folder holding its `kind` ('Registered' or 'Flow') files}, patients sorted"""
    if layout == "predict":
        found = {p: join(folder, p, kind) for p in sorted(os.listdir(folder))}
    elif layout == "saver":
        root = join(folder, "Postprocessed", kind)
        if not os.path.isdir(root):
            raise ValueError("%s: no Postprocessed/%s folder (the saver layout)" % (folder, kind))
        found = {p: join(root, p) for p in sorted(os.listdir(root))}
        if kind == "Registered":
            found = {p: join(d, "temp_allClasses") if os.path.isdir(join(d, "temp_allClasses")) else d for p, d in found.items()}
    else:
        raise ValueError("layout must be 'predict' or 'saver', got %r" % (layout,))
    return collections.OrderedDict((p, d) for p, d in found.items() if os.path.isdir(d))


def sorted_cases(folder, suffix):
    """the stems of the `suffix` files of a folder, sorted by frame number"""
    return sorted((_stem(f, suffix) for f in os.listdir(folder) if f.endswith(suffix)), key=frame_number)


def ed_es_indices(input_folder, patient):
    if input_folder is None:
        return 0, 0
    from .predict import get_ed_es_indices
    return get_ed_es_indices(join(input_folder, patient, patient + ".csv"))


def reference_name(stem, gt_mode, ed_index):
    """the GT case a predicted case is scored against: its own frame, or the ED frame's (frame digits <- ed_index + 1, zero-filled)"""
    if gt_mode == "frame":
        return stem
    if gt_mode == "ed":
        return stem[:-2] + str(ed_index + 1).zfill(2)
    raise ValueError("--gt must be 'frame' or 'ed', got %r" % (gt_mode,))


def pair_segmentation_cases(pred_folder, gt_folder, gt_mode="frame", ed_index=0):
    """Cases of one patient folder with their GT files, sorted by frame number; cases without a GT file are skipped."""
    cases = []
    for stem in sorted_cases(pred_folder, ".nii.gz"):
        gt = join(gt_folder, reference_name(stem, gt_mode, ed_index) + ".nii.gz")
        if os.path.isfile(gt):
            cases.append(Case(stem, frame_number(stem), join(pred_folder, stem + ".nii.gz"), gt))
    return cases


def label_file(label_folder, patient, stem):
    for cand in (join(label_folder, stem + ".nii.gz"), join(label_folder, patient, stem + ".nii.gz"),
                 join(label_folder, patient, "Segmentation", stem + ".nii.gz")):
        if os.path.isfile(cand):
            return cand
    return None


def _nifti_shape(path):
    """(Z, Y, X) from the header alone"""
    with open(path, "rb") as f:
        raw = f.read()
    head = zlib.decompressobj(wbits=31).decompress(raw, 352) if str(path).endswith(".gz") else raw[:352]
    dim = np.frombuffer(head, dtype="<i2", count=8, offset=40)
    return (max(int(dim[3]), 1) if dim[0] >= 3 else 1, max(int(dim[2]), 1), int(dim[1]))


def _npz_shape(path, key):
    with zipfile.ZipFile(path) as z, z.open(key + ".npy") as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        return tuple(read(f)[0])


def pair_jacobian_cases(flow_folder, label_folder, patient, ed_index=None):
    """Flow files of one patient with their label volumes, sorted by frame number, the ED frame's file (frame number ed_index + 1) left out
    when ed_index is known.  A missing or mis-shaped label volume is a ValueError naming the case (headers only: nothing is inflated)."""
    cases = []
    for stem in sorted_cases(flow_folder, ".npz"):
        if ed_index is not None and frame_number(stem) == ed_index + 1:
            continue
        lab = label_file(label_folder, patient, stem)
        if lab is None:
            raise ValueError("case %s: no label volume %s.nii.gz in %s (flat, per patient or <patient>/Segmentation)" % (stem, stem, label_folder))
        fshape = _npz_shape(join(flow_folder, stem + ".npz"), "flow")
        if len(fshape) != 4 or fshape[3] != 2:
            raise ValueError("case %s: flow of shape %s, expected [H, W, D, 2]" % (stem, fshape))
        Z, Y, X = _nifti_shape(lab)
        if (Y, X, Z) != fshape[:3]:
            raise ValueError("case %s: label volume %s is [Z, Y, X] = %s, the flow [H, W, D] = %s" % (stem, lab, (Z, Y, X), fshape[:3]))
        cases.append(Case(stem, frame_number(stem), join(flow_folder, stem + ".npz"), lab))
    return cases


def pair_ssim_cases(flow_folder, input_folder, patient, ed_index, label_folder=None):
    """-> [ED case] + the flow files of one patient sorted by frame number, the ED frame's own flow file (frame number ed_index + 1) left
    out as pair_jacobian_cases leaves it out; [] without flow files.  A flow case's `other` is its image
    INPUT/<patient>/<case>_0000.nii.gz; the ED case's `path` is the ED image and its `other` the ED label volume (label_file under the ED
    case's stem; None without a label folder).  A missing image, a missing ED label volume or an image / label volume whose [Z, Y, X] is
    not the flow's [H, W, D] is a ValueError naming the case (headers only: nothing is inflated)."""
    stems = [s for s in sorted_cases(flow_folder, ".npz") if frame_number(s) != ed_index + 1]
    if not stems:
        return []
    ed_stem = stems[0][:-2] + str(ed_index + 1).zfill(2)

    def image_of(stem):
        img = join(input_folder, patient, stem + "_0000.nii.gz")
        if not os.path.isfile(img):
            raise ValueError("case %s: no image %s" % (stem, img))
        return img
    lab = None
    if label_folder is not None:
        lab = label_file(label_folder, patient, ed_stem)
        if lab is None:
            raise ValueError("case %s: no label volume %s.nii.gz of the ED frame in %s (flat, per patient or <patient>/Segmentation)"
                             % (ed_stem, ed_stem, label_folder))
    cases = [Case(ed_stem, ed_index + 1, image_of(ed_stem), lab)]
    for stem in stems:
        cases.append(Case(stem, frame_number(stem), join(flow_folder, stem + ".npz"), image_of(stem)))
    want = None
    for c in cases[1:]:
        fshape = _npz_shape(c.path, "flow")
        if len(fshape) != 4 or fshape[3] != 2:
            raise ValueError("case %s: flow of shape %s, expected [H, W, D, 2]" % (c.name, fshape))
        if want is not None and fshape[:3] != want:
            raise ValueError("case %s: flow [H, W, D] = %s, the patient's other flows %s" % (c.name, fshape[:3], want))
        want = fshape[:3]
        Z, Y, X = _nifti_shape(c.other)
        if (Y, X, Z) != want:
            raise ValueError("case %s: image %s is [Z, Y, X] = %s, the flow [H, W, D] = %s" % (c.name, c.other, (Z, Y, X), want))
    for what, f in (("image", cases[0].path), ("label volume", lab)):
        if f is not None:
            Z, Y, X = _nifti_shape(f)
            if (Y, X, Z) != want:
                raise ValueError("case %s: %s %s is [Z, Y, X] = %s, the flow [H, W, D] = %s" % (ed_stem, what, f, (Z, Y, X), want))
    return cases


def _nifti_zooms(path):
    """pixdim[1:3] from the header alone: nibabel's header.get_zooms()[:2]"""
    with open(path, "rb") as f:
        raw = f.read()
    head = zlib.decompressobj(wbits=31).decompress(raw, 352) if str(path).endswith(".gz") else raw[:352]
    pixdim = np.frombuffer(head, dtype="<f4", count=8, offset=76)
    return float(pixdim[1]), float(pixdim[2])


def _npy_shape(path):
    with open(path, "rb") as f:
        version = np.lib.format.read_magic(f)
        read = np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0
        return tuple(read(f)[0])


def pair_contour_cases(flow_folder, contour_folder, input_folder, patient, ed_index):
    """-> (cases, zoom): the flow files of one patient sorted by frame number, the ED frame's own flow file (frame number ed_index + 1)
    left out, then one case per slice d whose `path` / `other` are contour/LV/<patient>_slice<d+1>.npy ([4, P, T]: endo x, y, epi x, y)
    and contour/RV/<patient>_slice<d+1>.npy ([2, P2, T]); zoom the in-plane spacing of the ED image INPUT/<patient>/<ED case>_0000.nii.gz.
    ([], None) without flow files.  With T - 1 flow files the frame numbers have to be 1 .. T without ed_index + 1 and every contour
    file has to hold T frames; a missing or mis-shaped file is a ValueError naming it (headers only: nothing is read)."""
    stems = [s for s in sorted_cases(flow_folder, ".npz") if frame_number(s) != ed_index + 1]
    if not stems:
        return [], None
    T = len(stems) + 1
    if [frame_number(s) for s in stems] != [t + 1 for t in range(T) if t != ed_index]:
        raise ValueError("patient %s: flow files of frames %s, expected 1 .. %d without the ED frame %d (ed_index %d)"
                         % (patient, [frame_number(s) for s in stems], T, ed_index + 1, ed_index))
    cases, want = [], None
    for stem in stems:
        path = join(flow_folder, stem + ".npz")
        fshape = _npz_shape(path, "flow")
        if len(fshape) != 4 or fshape[3] != 2:
            raise ValueError("case %s: flow of shape %s, expected [H, W, D, 2]" % (stem, fshape))
        if want is not None and fshape[:3] != want:
            raise ValueError("case %s: flow [H, W, D] = %s, the patient's other flows %s" % (stem, fshape[:3], want))
        want = fshape[:3]
        cases.append(Case(stem, frame_number(stem), path, None))
    for d in range(want[2]):
        name = "%s_slice%s" % (patient, str(d + 1).zfill(2))
        files = [join(contour_folder, "contour", k, name + ".npy") for k in ("LV", "RV")]
        for f, rows in zip(files, (4, 2)):
            if not os.path.isfile(f):
                raise ValueError("patient %s: no contour file %s (slice %d of %d)" % (patient, f, d, want[2]))
            shape = _npy_shape(f)
            if len(shape) != 3 or shape[0] != rows:
                raise ValueError("contour file %s: shape %s, expected [%d, P, T]%s" % (f, shape, rows, " (endo and epi points pair up)" if rows == 4 else ""))
            if shape[2] != T:
                raise ValueError("contour file %s: %d frames, but %d flow files + the ED frame = %d" % (f, shape[2], T - 1, T))
        cases.append(Case(name, d, files[0], files[1]))
    ed_stem = stems[0][:-2] + str(ed_index + 1).zfill(2)
    img = join(input_folder, patient, ed_stem + "_0000.nii.gz")
    if not os.path.isfile(img):
        raise ValueError("case %s: no image %s (the pixel spacing of the strain curves)" % (ed_stem, img))
    return cases, _nifti_zooms(img)


# ------------------------------------------------------------------------------------------------ host tables
def segmentation_row(name, scores):
    """one csv row (the thirteen columns) from {'RV': {'Dice', 'HD', 'ASSD'}, 'MYO': ..., 'LV': ...}"""
    row = {"Name": name}
    for m in SEG_METRICS:
        row["Average_" + m] = (scores["RV"][m] + scores["MYO"][m] + scores["LV"][m]) / 3
    for s in STRUCTURES:
        for m in SEG_METRICS:
            row["%s_%s" % (s, m)] = scores[s][m]
    return {k: row[k] for k in SEG_COLUMNS}


def segmentation_tables(cases):
    """cases: per-case dicts {'patient', 'name', 'test', 'reference', 'is_es', 'scores': {structure: {'Dice', 'HD', 'ASSD'}}} in patient and
    frame order -> (json document, csv rows, ES csv rows).  mean is np.nanmean over all cases, std is np.std (NaN as soon as one case is)."""
    doc = {"all": collections.OrderedDict(), "mean": {}, "std": {}}
    rows, es_rows, flat = [], [], []
    for c in cases:
        entry = {s: {m: float(c["scores"][s][m]) for m in SEG_METRICS} for s in STRUCTURES}
        entry["test"], entry["reference"] = c["test"], c["reference"]
        doc["all"].setdefault(c["patient"], []).append(entry)
        flat.append(entry)
        row = segmentation_row(c["name"], entry)
        rows.append(row)
        if c["is_es"]:
            es_rows.append(row)
    for s in STRUCTURES:
        doc["mean"][s], doc["std"][s] = {}, {}
        for m in SEG_METRICS:
            col = np.array([e[s][m] for e in flat], dtype=np.float64)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", category=RuntimeWarning)                    # an all-NaN or empty column: NaN, like numpy
                doc["mean"][s][m] = float(np.nanmean(col)) if col.size else float("nan")
                doc["std"][s][m] = float(np.std(col)) if col.size else float("nan")
    return doc, rows, es_rows


JACOBIAN_ES_KEYS = (("ES_negative_%", "negative_%"), ("ES_negative_%_average", "negative_%_average")) + \
    tuple(("ES_negative_%_average_" + k, "negative_%_" + k) for k in STRUCTURES)


def jacobian_rows(names, stats, es_position):
    """names[t]: case of frame position t; stats: cine_jacobian_table's dicts (slices outermost); es_position: position of the ES frame in
    `names` (None: no row is the ES row) -> the script's rows: Name, Slice nb, Frame nb, the gradients and statistics, and the five ES_*
    columns, which hold the row's own figures on the ES frame and NaN elsewhere."""
    T = len(names)
    assert len(stats) % T == 0
    rows = []
    for i, st in enumerate(stats):
        d, t = divmod(i, T)
        row = collections.OrderedDict([("Name", names[t]), ("Slice nb", float(d)), ("Frame nb", float(t))])
        row.update(st)
        for es_key, key in JACOBIAN_ES_KEYS:
            row[es_key] = row[key] if t == es_position else float("nan")
        rows.append(row)
    return rows


def jacobian_tables(rows):
    """rows of every patient -> the json document {'all': rows, 'mean': ...} with the script's `mean` keys: plain means (NaN as soon as one
    row is -- so the per-structure ES_negative_%_average_* means are NaN whenever a non-ES row exists), nanmeans for the two ES_*_mean
    keys, and the negative_% of the summed counts."""
    col = lambda k: np.array([r[k] for r in rows], dtype=np.float64)          # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        mean = collections.OrderedDict()
        mean["Temporal gradient"] = float(col("Temporal gradient").mean())
        mean["Spatial gradient"] = float(col("Spatial gradient").mean())
        mean["abs(Mean jacobian - 1)"] = float(col("abs(Mean jacobian - 1)").mean())
        mean["total_sum"] = float(col("total").sum())
        mean["negative_sum"] = float(col("negative").sum())
        mean["negative_%"] = float(np.float64(mean["negative_sum"]) / np.float64(mean["total_sum"]) * 100)
        mean["ES_negative_%_mean"] = float(np.nanmean(col("ES_negative_%")))
        mean["negative_%_mean"] = float(col("negative_%").mean())
        mean["negative_%_mean_average"] = float(col("negative_%_average").mean())
        mean["abs(Mean jacobian - 1)_average"] = float(col("abs(Mean jacobian - 1)_average").mean())
        mean["ES_negative_%_mean_average"] = float(np.nanmean(col("ES_negative_%_average")))
        for k in STRUCTURES:
            mean["negative_sum_" + k] = float(col("negative_" + k).sum())
            mean["total_sum_" + k] = float(col("total_" + k).sum())
            mean["negative_%_" + k] = float(np.float64(mean["negative_sum_" + k]) / np.float64(mean["total_sum_" + k]) * 100)
            mean["negative_%_mean_" + k] = float(col("negative_%_" + k).mean())
            mean["abs(Mean jacobian - 1)_" + k] = float(col("abs(Mean jacobian - 1)_" + k).mean())
            mean["ES_negative_%_average_" + k] = float(col("ES_negative_%_average_" + k).mean())
    return {"all": [dict(r) for r in rows], "mean": dict(mean)}


SSIM_KEYS = ("SSIM_mean",) + tuple("SSIM_" + k.lower() for k in STRUCTURES) + ("SSIM_whole",)
SSIM_COLUMNS = ["Name", "slice_number", "SSIM"]
SSIM_ALL_COLUMNS = ["Name", "slice_number"] + list(SSIM_KEYS) + ["ES_" + k for k in SSIM_KEYS]


def ssim_rows(patient, frames, stats, ed_frame, es_frame):
    """frames[t]: frame number of position t (ascending, the ED frame not among them); stats: cine_ssim_table's dicts (slices outermost)
    -> (entries, entries_all), one entry per slice.  The lists run over the frames by number, rotated to start with the first frame after
    ed_frame (the scripts' `indices >= ed` then `< ed`).  entries: Name, slice_number, SSIM (the whole-slice scores); entries_all (empty
    when the stats carry no structures): the five SSIM_* lists and ES_SSIM_*, the values of the frame numbered es_frame, NaN when that
    frame is not among `frames`."""
    T = len(frames)
    assert T and len(stats) % T == 0
    order = [t for t in range(T) if frames[t] > ed_frame] + [t for t in range(T) if frames[t] < ed_frame]
    es_position = frames.index(es_frame) if es_frame in frames else None
    entries, entries_all = [], []
    for d in range(len(stats) // T):
        st = stats[d * T:(d + 1) * T]
        entries.append(collections.OrderedDict([("Name", patient), ("slice_number", d), ("SSIM", [float(st[t]["SSIM_whole"]) for t in order])]))
        if "SSIM_mean" in st[0]:
            e = collections.OrderedDict([("Name", patient), ("slice_number", d)])
            for k in SSIM_KEYS:
                e[k] = [float(st[t][k]) for t in order]
            for k in SSIM_KEYS:
                e["ES_" + k] = float(st[es_position][k]) if es_position is not None else float("nan")
            entries_all.append(e)
    return entries, entries_all


def ssim_tables(entries, key="SSIM"):
    """entries of every patient -> (json document {'all': entries, 'mean': ...}, csv rows).  A csv row is the entry with every list
    replaced by its plain mean; `mean` is the plain mean over the entries of the per-entry means of `key` (NaN as soon as one value is)."""
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for e in entries:
            rows.append(collections.OrderedDict((k, float(np.array(v, dtype=np.float64).mean()) if isinstance(v, list) else v) for k, v in e.items()))
        mean = float(np.array([r[key] for r in rows], dtype=np.float64).mean()) if rows else float("nan")
    return {"all": [dict(e) for e in entries], "mean": mean}, rows


CONTOUR_STRUCTURES = ("ENDO", "EPI", "RV")
CONTOUR_COLUMNS = ["Name", "slice_number"] + list(CONTOUR_STRUCTURES) + ["Average"]
CONTOUR_MODES = ("from_ed", "from_ed_accumulation", "to_ed", "to_ed_accumulation")


def contour_rows(patient, errors):
    """errors [D, T - 1, 3] (strain.track_patient) -> the script's per-slice entries: Name, slice_number and the per-frame lists"""
    return [collections.OrderedDict([("Name", patient), ("slice_number", d)] + [(k, [float(v) for v in e[:, i]]) for i, k in enumerate(CONTOUR_STRUCTURES)])
            for d, e in enumerate(np.asarray(errors))]


def contour_tables(per_patient):
    """{patient: contour_rows} -> (json document, csv rows) as compute_contour_metrics.py:615-653 builds them: a csv row is the entry with
    every list replaced by its plain mean over the frames plus Average = (ENDO + EPI + RV) / 3; `mean` and `std` are numpy's plain mean
    and std of those per-slice means over all slices of all patients (NaN as soon as one slice has no points of the structure)."""
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for entries in per_patient.values():
            for e in entries:
                row = collections.OrderedDict((k, float(np.array(v, dtype=np.float64).mean()) if isinstance(v, list) else v) for k, v in e.items())
                row["Average"] = (row["ENDO"] + row["EPI"] + row["RV"]) / 3
                rows.append(row)
        col = lambda k: np.array([r[k] for r in rows], dtype=np.float64)          # noqa: E731
        doc = {"all": collections.OrderedDict((p, [dict(e) for e in entries]) for p, entries in per_patient.items()),
               "mean": {k: float(col(k).mean()) if rows else float("nan") for k in CONTOUR_STRUCTURES},
               "std": {k: float(col(k).std()) if rows else float("nan") for k in CONTOUR_STRUCTURES}}
    return doc, rows


def strain_rows(patient, curves, to_roll):
    """curves [D, T, 2] (strain.track_patient: radial, circumferential, ED first) -> per-slice entries with the curves rolled back by
    `to_roll` frames to the acquisition order (get_strain.py:588-589) and `smooth`, the mean of the two curvature variances (:596-599)."""
    from .strain import smoothness_measure
    entries = []
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for d, c in enumerate(np.asarray(curves, dtype=np.float64)):
            radial, circ = np.roll(c[:, 0], -to_roll), np.roll(c[:, 1], -to_roll)
            x = np.arange(len(radial))
            smooth = (smoothness_measure(x, radial) + smoothness_measure(x, circ)) / 2
            entries.append(collections.OrderedDict([("Name", patient), ("slice_number", d), ("radial_strain", [float(v) for v in radial]),
                                                    ("circ_strain", [float(v) for v in circ]), ("smooth", float(smooth))]))
    return entries


def strain_tables(per_patient):
    """{patient: strain_rows} -> {'all': ..., 'mean'}: `mean` the mean over the patients of each patient's mean smoothness over its slices
    (what get_strain.py:604 returns per patient and :681 prints)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        per = [float(np.array([e["smooth"] for e in entries], dtype=np.float64).mean()) for entries in per_patient.values()]
        mean = float(np.array(per, dtype=np.float64).mean()) if per else float("nan")
    return {"all": collections.OrderedDict((p, [dict(e) for e in entries]) for p, entries in per_patient.items()), "mean": mean}


def write_csv(file, columns, rows):
    with open(file, "w", newline="") as f:
        writer = csv.DictWriter(f, fieldnames=list(columns))
        writer.writeheader()
        writer.writerows(rows)


# ------------------------------------------------------------------------------------------------ readers (thread pool)
def _structure_labels(a, what):
    """label volume -> uint8 with every value other than 1, 2, 3 set to 0 (the scripts only ever ask `== 1`, `== 2`, `== 3`)"""
    a = np.asarray(a)
    if a.dtype.kind == "f" and not np.array_equal(a, np.rint(a)):
        raise ValueError("%s: not a label volume (non-integer values)" % what)
    return np.where((a >= 1) & (a <= len(STRUCTURES)), a, 0).astype(np.uint8)


def _read_seg_case(case):
    test, _ = read_nifti(case.path)
    ref, props = read_nifti(case.other)
    if test.shape != ref.shape:
        raise ValueError("case %s: prediction %s and reference %s differ in shape" % (case.name, test.shape, ref.shape))
    spacing = tuple(float(v) for v in props["itk_spacing"][::-1])                        # the GT header's zooms, in array order (z, y, x)
    return _structure_labels(test, case.path), _structure_labels(ref, case.other), spacing


def _read_jacobian_case(case):
    with np.load(case.path) as z:
        flow = np.asarray(z["flow"], dtype=np.float32)
    lab, _ = read_nifti(case.other)
    lab = _structure_labels(lab, case.other).transpose(1, 2, 0)                         # [Z, Y, X] -> the flow's [H, W, D]
    if lab.shape != flow.shape[:3] or flow.shape[3:] != (2,):
        raise ValueError("case %s: label volume %s and flow %s do not match" % (case.name, lab.shape, flow.shape))
    return flow, lab


def _read_ssim_case(case):
    """a flow case -> (flow fp32 [H, W, D, 2], image fp32 [H, W, D]); the ED case -> (image fp64 [H, W, D], labels uint8 [H, W, D] or None)"""
    if case.path.endswith(".npz"):
        with np.load(case.path) as z:
            flow = np.asarray(z["flow"], dtype=np.float32)
        img, _ = read_nifti(case.other)
        img = np.asarray(img).transpose(1, 2, 0).astype(np.float32)                     # [Z, Y, X] -> the flow's [H, W, D]
        if img.shape != flow.shape[:3] or flow.shape[3:] != (2,):
            raise ValueError("case %s: image %s and flow %s do not match" % (case.name, img.shape, flow.shape))
        return flow, img
    img, _ = read_nifti(case.path)
    lab = None
    if case.other is not None:
        lab = _structure_labels(read_nifti(case.other)[0], case.other).transpose(1, 2, 0)
    return np.asarray(img).transpose(1, 2, 0).astype(np.float64), lab


def _read_contour_case(case):
    """a flow case -> flow fp32 [H, W, D, 2]; a slice's contour case -> (lv [T, P, 4], rv [T, P2, 2]) as the script transposes them"""
    if case.path.endswith(".npz"):
        with np.load(case.path) as z:
            flow = np.asarray(z["flow"], dtype=np.float32)
        if flow.ndim != 4 or flow.shape[3] != 2:
            raise ValueError("case %s: flow of shape %s, expected [H, W, D, 2]" % (case.name, flow.shape))
        return flow
    lv, rv = np.load(case.path).transpose((2, 1, 0)), np.load(case.other).transpose((2, 1, 0))
    if lv.ndim != 3 or lv.shape[2] != 4 or rv.ndim != 3 or rv.shape[2] != 2 or len(lv) != len(rv):
        raise ValueError("contours %s: LV %s and RV %s, expected [4, P, T] and [2, P2, T]" % (case.name, lv.shape[::-1], rv.shape[::-1]))
    return lv, rv


def _prefetched(patients, read):
    """yields (patient, cases, [read(case)]) in order; the files of the next patient are read while the caller works on this one"""
    for (_, loaded), (patient, cases) in zip(read_ahead([cases for _, cases in patients], read, depth=1, readers=READERS), patients):
        yield patient, cases, loaded


# ------------------------------------------------------------------------------------------------ drivers
def score_segmentation_patient(loaded):
    """loaded: [(test, reference, spacing)] of one patient -> per case {structure: {'Dice', 'HD', 'ASSD'}}.  One device visit per group of
    frames that share shape and spacing (one group for a cine)."""
    from . import metrics
    groups = collections.OrderedDict()
    for i, (t, r, sp) in enumerate(loaded):
        groups.setdefault((t.shape, sp), []).append(i)
    out = [None] * len(loaded)
    for (_, sp), idx in groups.items():
        sc = metrics.cine_label_scores(np.stack([loaded[i][0] for i in idx]), np.stack([loaded[i][1] for i in idx]), len(STRUCTURES) + 1,
                                       voxel_spacing=sp, reproducible=True)
        for n, i in enumerate(idx):
            out[i] = {s: {"Dice": float(sc["dice"][n, c]), "HD": float(sc["hd"][n, c]), "ASSD": float(sc["assd"][n, c])}
                      for c, s in enumerate(STRUCTURES, 1)}
    return out


def score_segmentation(pred, ref, input_folder=None, gt="frame", layout="predict"):
    """The `seg` sub-command.  Returns the json document; the three files are written into `pred`.  The ES row is the case whose frame
    number is es_index + 1."""
    patients, es_frame = [], {}
    for patient, folder in patient_folders(pred, layout, "Registered").items():
        ed, es = ed_es_indices(input_folder, patient)
        cases = pair_segmentation_cases(folder, ref, gt, ed)
        if cases:
            patients.append((patient, cases))
            es_frame[patient] = es + 1
    per_case = []
    for patient, cases, loaded in _prefetched(patients, _read_seg_case):
        for case, scores in zip(cases, score_segmentation_patient(loaded)):
            per_case.append({"patient": patient, "name": case.name, "test": case.path, "reference": case.other,
                             "is_es": case.frame == es_frame[patient], "scores": scores})
    doc, rows, es_rows = segmentation_tables(per_case)
    save_json(doc, join(pred, "segmentation_metrics.json"))
    write_csv(join(pred, "segmentation_metrics.csv"), SEG_COLUMNS, rows)
    write_csv(join(pred, "segmentation_metrics_es.csv"), SEG_COLUMNS, es_rows)
    return doc


def score_jacobian(flow, labels, input_folder=None, layout="predict"):
    """The `jacobian` sub-command.  Returns the json document; jacobian.json and jacobian_metrics.csv are written into `flow`."""
    from . import metrics
    patients, es_frame = [], {}
    for patient, folder in patient_folders(flow, layout, "Flow").items():
        ed, es = ed_es_indices(input_folder, patient)
        cases = pair_jacobian_cases(folder, labels, patient, ed if input_folder is not None else None)
        if cases:
            patients.append((patient, cases))
            es_frame[patient] = es + 1
    rows = []
    for patient, cases, loaded in _prefetched(patients, _read_jacobian_case):
        if len({f.shape for f, _ in loaded}) != 1:
            raise ValueError("patient %s: the flow files differ in shape" % patient)
        stats = metrics.cine_jacobian_table(np.stack([f for f, _ in loaded]), np.stack([g for _, g in loaded]), STRUCTURES)
        frames = [c.frame for c in cases]
        es_position = frames.index(es_frame[patient]) if es_frame[patient] in frames else None
        rows += jacobian_rows([c.name for c in cases], stats, es_position)
    if not rows:
        raise ValueError("%s: no flow files found (layout %r)" % (flow, layout))
    doc = jacobian_tables(rows)
    save_json(doc, join(flow, "jacobian.json"))
    write_csv(join(flow, "jacobian_metrics.csv"), list(rows[0].keys()), rows)
    return doc


def score_ssim(flow, input_folder, labels=None, layout="predict", win=7):
    """The `ssim` sub-command.  Returns the json document of ssim_metrics.json; ssim_metrics.{json,csv} are written into `flow`, and with
    a label folder ssim_metrics_all.{json,csv} as well.  Every frame with a flow file is warped onto the ED frame with that file's flow
    and scored against the ED image: two library calls per patient."""
    from . import metrics
    patients, es_frame = [], {}
    for patient, folder in patient_folders(flow, layout, "Flow").items():
        ed, es = ed_es_indices(input_folder, patient)
        cases = pair_ssim_cases(folder, input_folder, patient, ed, labels)
        if cases:
            patients.append((patient, cases))
            es_frame[patient] = es + 1
    entries, entries_all = [], []
    for patient, cases, loaded in _prefetched(patients, _read_ssim_case):
        (fixed, lab), moving = loaded[0], loaded[1:]
        stats = metrics.cine_ssim_table(fixed, np.stack([m for _, m in moving]), np.stack([f for f, _ in moving]), lab, STRUCTURES, win)
        e, ea = ssim_rows(patient, [c.frame for c in cases[1:]], stats, cases[0].frame, es_frame[patient])
        entries += e
        entries_all += ea
    if not entries:
        raise ValueError("%s: no flow files found (layout %r)" % (flow, layout))
    doc, rows = ssim_tables(entries, "SSIM")
    save_json(doc, join(flow, "ssim_metrics.json"))
    write_csv(join(flow, "ssim_metrics.csv"), SSIM_COLUMNS, rows)
    if labels is not None:
        doc_all, rows_all = ssim_tables(entries_all, "SSIM_mean")
        save_json(doc_all, join(flow, "ssim_metrics_all.json"))
        write_csv(join(flow, "ssim_metrics_all.csv"), SSIM_ALL_COLUMNS, rows_all)
    return doc


def contour_arrays(flows, contours, ed_index):
    """flows: the T - 1 arrays [H, W, D, 2] by frame number without the ED frame; contours: per slice (lv [T, P, 4], rv [T, P2, 2]),
    1-based, in acquisition order -> (flow [D, T, 2, W, H], pts [D, T, Pmax, 2], counts [D, 3]) in ED-first order, the points 0-based:
    what every mode of compute_contour_metrics.py prepares before its loops."""
    from . import strain
    flow, idx = strain.prepare_flow(flows, ed_index)
    if len(contours) != len(flow):
        raise ValueError("%d contour slices for a flow of %d slices" % (len(contours), len(flow)))
    per_slice = [(lv[idx, :, :2] - 1, lv[idx, :, 2:] - 1, rv[idx] - 1) for lv, rv in contours]
    pts, counts = strain.pack_contours(per_slice)
    return flow, pts, counts


def score_contour(flow, contours, input_folder, layout="predict", mode="from_ed"):
    """The `contour` sub-command.  Returns the json document of contour_metrics.json; contour_metrics.{json,csv} are written into `flow`,
    and strain_metrics.json in mode from_ed.  One upload, at most two library calls and one download per patient (strain.track_patient)."""
    from . import metrics, strain
    if mode not in CONTOUR_MODES:
        raise ValueError("--mode must be one of %s, got %r" % (", ".join(CONTOUR_MODES), mode))
    patients, info = [], {}
    for patient, folder in patient_folders(flow, layout, "Flow").items():
        ed, _ = ed_es_indices(input_folder, patient)
        cases, zoom = pair_contour_cases(folder, contours, input_folder, patient, ed)
        if cases:
            patients.append((patient, cases))
            info[patient] = (ed, zoom)
    errors, curves = collections.OrderedDict(), collections.OrderedDict()
    for patient, cases, loaded in _prefetched(patients, _read_contour_case):
        nflow = sum(1 for c in cases if c.path.endswith(".npz"))
        ed, zoom = info[patient]
        f, pts, counts = contour_arrays(loaded[:nflow], loaded[nflow:], ed)
        with_strain = mode == "from_ed"
        metrics.contour_counts(counts, len(pts), pts.shape[2], strain=with_strain)          # refusals before any device work
        res = strain.track_patient(f, pts, counts, mode, np.asarray(zoom, dtype=np.float32) if with_strain else None)
        errors[patient] = contour_rows(patient, res["errors"])
        if with_strain:
            curves[patient] = strain_rows(patient, res["strain"], pts.shape[1] - ed)
    if not errors:
        raise ValueError("%s: no flow files found (layout %r)" % (flow, layout))
    doc, rows = contour_tables(errors)
    save_json(doc, join(flow, "contour_metrics.json"))
    write_csv(join(flow, "contour_metrics.csv"), CONTOUR_COLUMNS, rows)
    if curves:
        save_json(strain_tables(curves), join(flow, "strain_metrics.json"))
    return doc


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Score the folders of a cine prediction on the device, one visit per patient.")
    sub = parser.add_subparsers(dest="command", required=True)
    seg = sub.add_parser("seg", help="Dice / HD / ASSD of the propagated labels: segmentation_metrics.{json,csv}, segmentation_metrics_es.csv")
    seg.add_argument("-pred", required=True, help="output folder of the prediction (one sub-folder per patient); the tables are written here")
    seg.add_argument("-ref", required=True, help="folder of the ground-truth label files <case>.nii.gz")
    seg.add_argument("--gt", choices=("frame", "ed"), default="frame", help="score a frame against its own GT, or every frame against the ED frame's")
    jac = sub.add_parser("jacobian", help="Jacobian statistics and flow gradients per slice and frame: jacobian.json, jacobian_metrics.csv")
    jac.add_argument("-flow", required=True, help="output folder of the prediction (one sub-folder per patient); the tables are written here")
    jac.add_argument("-l", required=True, help="folder of the label volumes <case>.nii.gz, flat or per patient")
    for p in (seg, jac):
        p.add_argument("-i", default=None, help="input folder with <patient>/<patient>.csv (ed_index, es_index); without it both are 0")
        p.add_argument("--layout", choices=("predict", "saver"), default="predict")
    ssim = sub.add_parser("ssim", help="SSIM of every frame warped onto the ED frame: ssim_metrics.{json,csv}, with -l ssim_metrics_all.{json,csv}")
    ssim.add_argument("-flow", required=True, help="output folder of the prediction (one sub-folder per patient); the tables are written here")
    ssim.add_argument("-i", required=True, help="input folder with <patient>/<case>_0000.nii.gz and <patient>/<patient>.csv (ed_index, es_index)")
    ssim.add_argument("-l", default=None, help="folder of the label volumes <case>.nii.gz, flat or per patient: per-structure scores on the ED labels")
    ssim.add_argument("--layout", choices=("predict", "saver"), default="predict")
    ssim.add_argument("--win", type=int, default=7, help="side of the uniform SSIM window (odd, 3..15)")
    con = sub.add_parser("contour", help="tracking error of the ground-truth contour points under the flow: contour_metrics.{json,csv}; "
                                         "in mode from_ed also the strain curves: strain_metrics.json")
    con.add_argument("-flow", required=True, help="output folder of the prediction (one sub-folder per patient); the tables are written here")
    con.add_argument("-c", required=True, help="folder with contour/LV/<patient>_sliceNN.npy [4, P, T] and contour/RV/<patient>_sliceNN.npy [2, P2, T]")
    con.add_argument("-i", required=True, help="input folder with <patient>/<case>_0000.nii.gz and <patient>/<patient>.csv (ed_index, es_index)")
    con.add_argument("--layout", choices=("predict", "saver"), default="predict")
    con.add_argument("--mode", choices=CONTOUR_MODES, default="from_ed", help="the script's motion model (from_ed: its fallback without a training config)")
    return parser


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.command == "seg":
        return score_segmentation(a.pred, a.ref, a.i, a.gt, a.layout)
    if a.command == "jacobian":
        return score_jacobian(a.flow, a.l, a.i, a.layout)
    if a.command == "contour":
        return score_contour(a.flow, a.c, a.i, a.layout, a.mode)
    return score_ssim(a.flow, a.i, a.l, a.layout, a.win)


if __name__ == "__main__":
    main()
