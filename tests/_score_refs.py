"""Reference restatements for the cine tables (cineflow.score, csrc/score.hip), built from oracle.metrics alone: what the reference's
compute_metrics.py / compute_jacobian.py compute frame by frame and class by class, as plain numpy on the host.  Test infrastructure."""
import warnings

import numpy as np

from oracle import metrics as OM

NAMES = ("RV", "MYO", "LV")


def seg_scores(test, ref, spacing):
    """test / ref: one frame's label arrays -> {structure: {'Dice', 'HD', 'ASSD'}} (compute_metrics.py:96-106)"""
    out = {}
    for c, name in enumerate(NAMES, 1):
        a, b = test == c, ref == c
        out[name] = {"Dice": OM.dice(a, b), "HD": OM.hausdorff_distance(a, b, voxel_spacing=spacing),
                     "ASSD": OM.avg_surface_distance_symmetric(a, b, voxel_spacing=spacing)}
    return out


def frame_stats(frame_flow, frame_gt, names=NAMES):
    """oracle.metrics.jacobian_frame_stats; where a structure is absent the oracle (like the script) divides by zero, and the rows hold
    NaN for that structure's mean and percentage instead -- the rule of cineflow.metrics.jacobian_frame_stats"""
    if all((frame_gt == i).any() for i in range(1, len(names) + 1)):
        return OM.jacobian_frame_stats(frame_flow, frame_gt, names)
    jac = OM.jacobian_determinant(frame_flow)
    res = {}
    for i, k in enumerate(names, 1):
        cur = jac[frame_gt == i]
        total, neg = float(cur.size), float((cur < 0).sum())
        res["abs(Mean jacobian - 1)_" + k] = abs(cur.mean() - 1) if total else float("nan")
        res["total_" + k] = total
        res["negative_" + k] = neg
        res["negative_%_" + k] = (neg / total) * 100 if total else float("nan")
    res["abs(Mean jacobian - 1)_average"] = sum(res["abs(Mean jacobian - 1)_" + k] for k in names) / 3
    res["negative_%_average"] = sum(res["negative_%_" + k] for k in names) / 3
    res["abs(Mean jacobian - 1)"] = abs(jac.mean() - 1)
    res["total"] = float(jac.size)
    res["negative"] = float((jac < 0).sum())
    res["negative_%"] = (res["negative"] / res["total"]) * 100
    return res


def jacobian_rows(flow, labels, names=NAMES):
    """flow [T, H, W, D, 2], labels [T, H, W, D] -> (rows, near): one dict per (slice, frame), slices outermost, with the gradients of
    oracle.metrics.gradient_means and the statistics of frame_stats; near[i] = number of oracle determinants of that slice within 2e-5 of
    zero (the determinants that may change side under another rounding)."""
    T, H, W, D, _ = flow.shape
    rows, near = [], []
    for d in range(D):
        tg, sg = OM.gradient_means(flow[:, :, :, d])
        for t in range(T):
            row = {"Temporal gradient": float(tg[t]), "Spatial gradient": float(sg[t])}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", category=RuntimeWarning)
                row.update(frame_stats(flow[t, :, :, d], labels[t, :, :, d], names))
            rows.append(row)
            near.append(int((np.abs(OM.jacobian_determinant(flow[t, :, :, d])) <= 2e-5).sum()))
    return rows, near


def check_jacobian_row(got, want, near, tag=""):
    """the bars tests/test_metrics.py holds the per-frame functions to: means 1e-4, gradient means 1e-6, percentages 0.5; counts within
    the number of near-zero oracle determinants of the slice.  NaN must meet NaN.  Returns the worst figure of each kind."""
    worst = {"mean": 0.0, "gradient": 0.0, "percent": 0.0, "count": 0.0}
    assert set(want) <= set(got), (tag, set(want) - set(got))
    for k, w in want.items():
        g = got[k]
        if np.isnan(w):
            assert np.isnan(g), (tag, k, g)
            continue
        assert not np.isnan(g), (tag, k)
        err = abs(g - w)
        if k in ("Temporal gradient", "Spatial gradient"):
            kind, bar = "gradient", 1e-6
        elif k.startswith("total") or (k.startswith("negative") and "%" not in k):
            kind, bar = "count", near
        elif "%" in k:
            kind, bar = "percent", 0.5
        else:
            kind, bar = "mean", 1e-4
        worst[kind] = max(worst[kind], err)
        assert err <= bar, (tag, k, g, w, bar)
    return worst


def smooth_flow(rng, T, H, W, D, amplitude):
    """a random flow [T, H, W, D, 2], lightly smoothed along H and W so that determinants are not all noise"""
    f = rng.normal(size=(T, H, W, D, 2))
    for ax in (1, 2):
        if f.shape[ax] > 2:
            f = (np.roll(f, 1, ax) + f + np.roll(f, -1, ax)) / 3.0
    return (f * amplitude).astype(np.float32)


def structure_labels(rng, shape):
    """labels 0..3 drawn per pixel (every structure present when the map is large enough)"""
    return rng.integers(0, 4, size=shape).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ synthetic patients and their folders
def make_patient(seed, T, D=3, H=24, W=20, classes=(1, 2, 3), amplitude=1.6):
    """-> dict(gt, reg: uint8 [T, D, H, W] in file order (Z, Y, X); flow: float32 [T, H, W, D, 2]).  gt: an LV disc (3) inside a MYO ring
    (2) beside an RV disc (1), radii changing with the frame and the slice; reg: the same figure one pixel off with other radii."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def figure(t, z, dy, dx, grow):
        lab = np.zeros((H, W), np.uint8)
        cy, cx = H / 2 + dy, W / 2 + 2 + dx
        r = np.hypot(yy - cy, xx - cx)
        r1 = 2.5 + 0.4 * ((t + z) % 3) + grow
        if 1 in classes:
            lab[np.hypot(yy - cy, xx - (cx - 8)) <= 2.6 + 0.3 * (t % 2) + grow] = 1
        if 2 in classes:
            lab[r <= r1 + 2.2] = 2
        if 3 in classes:
            lab[r <= r1] = 3
        return lab
    gt = np.stack([np.stack([figure(t, z, 0, 0, 0.0) for z in range(D)]) for t in range(T)])
    reg = np.stack([np.stack([figure(t, z, 1, -1, 0.35) for z in range(D)]) for t in range(T)])
    return {"gt": gt, "reg": reg, "flow": smooth_flow(rng, T, H, W, D, amplitude)}


def case_names(patient, T):
    return ["%s_frame%02d" % (patient, t + 1) for t in range(T)]


def write_tree(root, layout, patient, data, ed, es, spacing=(1.25, 1.25, 10.0)):
    """Writes one patient in a layout under root/out, its GT under root/gt, its csv under root/input.  predict: every frame has Registered /
    Flow / Segmentation files; saver: the ED frame has a Segmentation file only, Registered files sit in temp_allClasses beside unfiltered
    copies (all zero, so a reader that takes the wrong ones is found out)."""
    import os
    from cineflow.nifti import write_nifti
    T = len(data["gt"])
    names = case_names(patient, T)
    out = os.path.join(root, "out")
    if layout == "predict":
        dirs = {k: os.path.join(out, patient, k) for k in ("Registered", "Flow", "Segmentation")}
        reg_dir = dirs["Registered"]
    else:
        dirs = {k: os.path.join(out, "Postprocessed", k, patient) for k in ("Registered", "Flow", "Segmentation")}
        reg_dir = os.path.join(dirs["Registered"], "temp_allClasses")
    for d in list(dirs.values()) + [reg_dir, os.path.join(root, "gt"), os.path.join(root, "input", patient)]:
        os.makedirs(d, exist_ok=True)
    for t, name in enumerate(names):
        write_nifti(os.path.join(root, "gt", name + ".nii.gz"), data["gt"][t], spacing=spacing)
        write_nifti(os.path.join(dirs["Segmentation"], name + ".nii.gz"), data["gt"][t], spacing=spacing)
        if layout == "saver" and t == ed:
            continue
        write_nifti(os.path.join(reg_dir, name + ".nii.gz"), data["reg"][t], spacing=spacing)
        if layout == "saver":
            write_nifti(os.path.join(dirs["Registered"], name + ".nii.gz"), np.zeros_like(data["reg"][t]), spacing=spacing)
        np.savez(os.path.join(dirs["Flow"], name + ".npz"), flow=data["flow"][t], spacing=np.asarray(spacing))
    with open(os.path.join(root, "input", patient, patient + ".csv"), "w") as f:
        f.write("ed_index,es_index\n%d,%d\n" % (ed, es))
    return out, os.path.join(root, "gt"), os.path.join(root, "input")
