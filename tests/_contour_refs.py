"""Restatements of nnunet/compute_contour_metrics.py (from_ed :478-527, from_ed_accumulation :105-131, to_ed_accumulation :214-249, to_ed
:335-392, the documents :615-653) and of nnunet/get_strain.py:531-599 for one slice, in numpy / torch on the CPU: fp32 sampling through
_kernel_refs.sample_points (F.grid_sample) and fp32 chain steps, then fp64 error and strain arithmetic on the fp32 positions.  `sampler`
is replaceable, so that a GPU test can walk the same chains with ops.sample_points and hold the table kernels to these functions on the
device's own positions.  Test infrastructure (tests/test_contour_cpu.py pins it to tests/golden/strain.npz)."""
import collections
import csv
import os

import numpy as np
import torch

from _kernel_refs import sample_points

MODES = ("from_ed", "from_ed_accumulation", "to_ed_accumulation", "to_ed")          # cf_contour_track_table's numbering
STRUCTURES = ("ENDO", "EPI", "RV")


def cpu_sampler(frame, xy):
    """frame fp32 [2, A, B], xy fp32 [P, 2] -> the flow at the points, fp32 [P, 2] (SpatialTransformerContour)"""
    out = sample_points(torch.as_tensor(frame)[None].float(), torch.as_tensor(xy).float().t()[None].contiguous())
    return out[0].t().contiguous()


def device_sampler(dev):
    """cpu_sampler's contract with one cineflow.ops.sample_points call per step on `dev` (the per-launch path of cineflow.strain)"""
    from cineflow import ops

    def sampler(frame, xy):
        out = ops.sample_points(frame[None].to(dev).contiguous(), xy.t()[None].contiguous().to(dev))
        return out[0].t().contiguous().cpu()
    return sampler


def positions(slice_flow, con, mode, sampler=cpu_sampler):
    """slice_flow [T, 2, A, B] (ED first; frame 0 is never read), con [T, P, 2] 0-based, same order -> fp32 [T - 1, P, 2]: what the script
    subtracts from the ground truth at output row t - 1 -- the tracked position (from_ed*) or the predicted delta (to_ed*).  The to_ed*
    loops run on reversed frames and flip their rows back; stated on the unreversed arrays: row t - 1 starts from the points of frame t
    and goes through flows t, t - 1, .., 1 (to_ed_accumulation) or flow t alone (to_ed)."""
    flow = torch.as_tensor(np.ascontiguousarray(slice_flow)).float()
    con = torch.as_tensor(np.ascontiguousarray(con)).float()
    T = len(flow)
    rows = []
    if mode == "from_ed":
        for t in range(1, T):
            rows.append(con[0] + sampler(flow[t], con[0]))                          # :513-514
    elif mode == "from_ed_accumulation":
        cur = con[0]
        for t in range(1, T):
            cur = cur + sampler(flow[t], cur)                                       # :116-117, one chain, an error at every t
            rows.append(cur)
    elif mode == "to_ed_accumulation":
        for t in range(1, T):
            cur = con[t]
            for t2 in range(t, 0, -1):
                cur = cur + sampler(flow[t2], cur)                                  # :231-234
            rows.append(cur - con[t])                                               # :236
    elif mode == "to_ed":
        for t in range(1, T):
            rows.append(sampler(flow[t], con[t]))                                   # :378
    else:
        raise ValueError(mode)
    return torch.stack(rows).numpy()


def point_errors(con, pos, mode):
    """fp64 [T - 1, P]: || ground truth - pos || per point, the ground truth being the points of frame t (from_ed*) or the delta
    (points of frame 0) - (points of frame t) (to_ed*), all from the fp32 values"""
    con = np.asarray(con, dtype=np.float32).astype(np.float64)
    gt = con[1:] if mode.startswith("from_ed") else con[0][None] - con[1:]
    return np.linalg.norm(gt - np.asarray(pos, dtype=np.float32).astype(np.float64), axis=2)


def error_table(con, pos, counts, mode):
    """fp64 [T - 1, 3]: np.split at cumsum(counts[:2]) and the mean of every part (:526-527); NaN for an empty structure"""
    n = int(np.sum(counts))
    e = point_errors(np.asarray(con)[:, :n], np.asarray(pos)[:, :n], mode)
    parts = np.split(e, np.cumsum(counts[:2]), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([x.sum(-1) / x.shape[1] for x in parts], axis=-1)


def strain_table(pos, ed, n, zoom):
    """get_strain.py:571-586 in fp64, unrolled: pos fp32 [T - 1, P, 2] (from_ed positions), ed fp32 [P, 2], endo = points [0, n), epi =
    [n, 2n), zoom (mm, mm) -> fp64 [T, 2] (radial, circumferential), ED first; 0 / 0 gives NaN"""
    pts = np.concatenate([np.asarray(ed, np.float32)[None], np.asarray(pos, np.float32)], axis=0).astype(np.float64)
    pts = pts * np.asarray(zoom, dtype=np.float32).astype(np.float64).reshape(1, 1, 2)
    endo, epi = pts[:, :n], pts[:, n:2 * n]
    with np.errstate(invalid="ignore", divide="ignore"):
        radial = np.linalg.norm(epi - endo, axis=2)                                                      # T, n
        radial_strain = 0.5 * ((radial ** 2 - radial[0][None] ** 2) / radial[0][None] ** 2)
        step = lambda c: np.linalg.norm(np.roll(c, -1, axis=1) - c, axis=2)                              # noqa: E731  closed contour
        circ = (step(endo) + step(epi)) / 2
        circ_strain = 0.5 * ((circ ** 2 - circ[0][None] ** 2) / circ[0][None] ** 2)
        return np.stack([radial_strain.sum(-1) / n, circ_strain.sum(-1) / n], axis=-1)


def curvature(x, y):
    """get_strain.py:26-32"""
    dx, dy = np.gradient(x), np.gradient(y)
    d2x, d2y = np.gradient(dx), np.gradient(dy)
    return np.abs((dx * d2y - dy * d2x) / ((dx ** 2 + dy ** 2) ** (3 / 2)))


def smoothness(curve):
    return float(np.var(curvature(np.arange(len(curve)), np.asarray(curve, dtype=np.float64))))


# ------------------------------------------------------------------------------------------------ folders
def make_contours(seed, T, D, H, W, counts=None):
    """per slice (lv [4, P, T], rv [2, P2, T]) as the reference's files hold them: 1-based points on noisy rings inside an [H, W, D] flow
    (coordinate 0 runs along H: the scripts' flow is [D, T, 2, W, H]); counts[d] = (P, P2), different per slice by default"""
    rng = np.random.default_rng(seed)
    out = []
    for d in range(D):
        P, P2 = counts[d] if counts is not None else (9 + 2 * d, 5 + d)
        ang, ang2 = np.linspace(0, 2 * np.pi, P, endpoint=False), np.linspace(0, 2 * np.pi, P2, endpoint=False)
        lv, rv = np.zeros((4, P, T)), np.zeros((2, P2, T))
        for t in range(T):
            k = 1.0 - 0.15 * np.sin(np.pi * t / T)
            for j, r in enumerate((0.18, 0.30)):
                lv[2 * j, :, t] = 1 + H * (0.5 + r * k * np.cos(ang)) + rng.normal(0, 0.2, P)
                lv[2 * j + 1, :, t] = 1 + W * (0.55 + r * k * np.sin(ang)) + rng.normal(0, 0.2, P)
            rv[0, :, t] = 1 + H * (0.5 + 0.12 * k * np.cos(ang2)) + rng.normal(0, 0.2, P2)
            rv[1, :, t] = 1 + W * (0.2 + 0.12 * k * np.sin(ang2)) + rng.normal(0, 0.2, P2)
        out.append((lv, rv))
    return out


def write_contours(root, patient, contours, skip=()):
    """<root>/contours/contour/{LV,RV}/<patient>_sliceNN.npy, NN = slice + 1; returns <root>/contours"""
    folder = os.path.join(root, "contours")
    for k in ("LV", "RV"):
        os.makedirs(os.path.join(folder, "contour", k), exist_ok=True)
    for d, (lv, rv) in enumerate(contours):
        name = "%s_slice%s.npy" % (patient, str(d + 1).zfill(2))
        if ("LV", d) not in skip:
            np.save(os.path.join(folder, "contour", "LV", name), lv)
        if ("RV", d) not in skip:
            np.save(os.path.join(folder, "contour", "RV", name), rv)
    return folder


def patient_tables(flow_files, contour_folder, patient, ed, zoom, mode, sampler=cpu_sampler):
    """One patient as the scripts walk it: flow_files = the .npz files by frame number WITHOUT the ED frame's; -> (errors [D, T - 1, 3],
    strain [D, T, 2] or None, to_roll).  compute_contour_metrics.py:47-100, get_strain.py:454-524."""
    video = [np.load(f)["flow"].transpose((2, 3, 0, 1)) for f in flow_files]                     # D, C, H, W
    flow = np.stack(video, axis=1).transpose(0, 1, 2, 4, 3)                                       # D, T, C, W, H
    flow = np.insert(flow, ed, values=np.nan, axis=1)
    frames = np.arange(flow.shape[1])
    frames = np.concatenate([frames[frames >= ed], frames[frames < ed]])
    to_roll = int((np.arange(flow.shape[1]) >= ed).sum())
    flow = flow[:, frames]
    errors, curves = [], []
    for d in range(len(flow)):
        name = "%s_slice%s.npy" % (patient, str(d + 1).zfill(2))
        lv = np.load(os.path.join(contour_folder, "contour", "LV", name)).transpose((2, 1, 0))   # T, P, 4
        rv = np.load(os.path.join(contour_folder, "contour", "RV", name)).transpose((2, 1, 0))   # T, P2, 2
        counts = (lv.shape[1], lv.shape[1], rv.shape[1])
        con = (np.concatenate([lv[:, :, :2], lv[:, :, 2:], rv], axis=1)[frames] - 1).astype(np.float32)
        pos = positions(flow[d], con, mode, sampler)
        errors.append(error_table(con, pos, counts, mode))
        if mode == "from_ed":
            curves.append(strain_table(pos, con[0], counts[0], zoom))
    return np.stack(errors), (np.stack(curves) if curves else None), to_roll


def documents(per_patient):
    """per_patient: {patient: (errors, strain or None, to_roll)} -> (contour_metrics.json document, csv rows, strain_metrics.json document
    or None): compute_contour_metrics.py:139-146 and :615-653, get_strain.py:588-604 and :681"""
    doc = {"all": collections.OrderedDict(), "mean": {}, "std": {}}
    rows, per_slice = [], {k: [] for k in STRUCTURES}
    sdoc, smooth_per_patient = {"all": collections.OrderedDict()}, []
    for patient, (errors, curves, to_roll) in per_patient.items():
        doc["all"][patient] = []
        for d, e in enumerate(errors):
            entry = {"Name": patient, "slice_number": d}
            entry.update({k: e[:, i].tolist() for i, k in enumerate(STRUCTURES)})
            doc["all"][patient].append(entry)
            row = dict(entry)
            for k in STRUCTURES:
                row[k] = np.array(entry[k]).mean()
                per_slice[k].append(row[k])
            row["Average"] = (row["ENDO"] + row["EPI"] + row["RV"]) / 3
            rows.append(row)
        if curves is not None:
            sdoc["all"][patient] = []
            for d, c in enumerate(curves):
                radial, circ = np.roll(c[:, 0], -to_roll), np.roll(c[:, 1], -to_roll)
                with np.errstate(invalid="ignore", divide="ignore"):
                    smooth = (smoothness(radial) + smoothness(circ)) / 2
                sdoc["all"][patient].append({"Name": patient, "slice_number": d, "radial_strain": radial.tolist(), "circ_strain": circ.tolist(),
                                             "smooth": smooth})
            smooth_per_patient.append(np.array([e["smooth"] for e in sdoc["all"][patient]]).mean())
    doc["mean"] = {k: float(np.array(per_slice[k]).mean()) for k in STRUCTURES}
    doc["std"] = {k: float(np.array(per_slice[k]).std()) for k in STRUCTURES}
    if not smooth_per_patient:
        return doc, rows, None
    sdoc["mean"] = float(np.array(smooth_per_patient).mean())
    return doc, rows, sdoc


def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))
