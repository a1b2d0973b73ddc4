"""Surface metrics of a 3-D case: the evaluator's EDT route (one cf_label_surface_edt visit per case) against the pairs route (borders compacted
and searched all-pairs, six times per label), and the sweep over object size that fixes metrics.EDT_AUTO_PAIRS.

Workload (default): one synthetic case of 160 x 384 x 384 voxels at spacing (2.5, 0.78125, 0.78125) with five ellipsoidal organs of differing
size (labels 1..5; the prediction is the reference with every organ shifted and rescaled a little), both volumes in host memory as the
evaluator has them after reading the files.

    (a) case     Evaluator(labels=[1..5]).evaluate(test, ref, advanced=True, surface=route) for route in edt, pairs: wall time with a device
                 synchronise at the end, one warm-up pair, then --runs pairs sampled alternately; medians and every sample; the library calls
                 of one evaluation per route, by name; the worst difference between the two routes' numbers
    (b) sweep    two offset balls of growing radius in a box that just holds them: hausdorff_distance (two directed distance vectors) per
                 route, alternately, --runs samples each; na x nb of every point and whether the transform won EVERY repeat; the constant is
                 the smallest power of two >= na x nb of the first point from which it does so at every larger point too
    (c) passes   --passes N: N cf_edt calls on the case's border mask and nothing else -- the run to put under `rocprofv3 --kernel-trace
                 --stats`; prints the bytes each pass must move.  --stats FILE reads that run's kernel_stats.csv and prints the achieved
                 bytes/s of each pass against the measured HBM copy rate (6.29 TB/s, MI355X_MICROARCH.md).  --visit N: N
                 label_surface_edt_table calls on device-resident volumes, for the same kind of trace (time per kernel only).

    python tools/edt_bench.py [--runs 5] [--small] [--no-sweep]            one JSON line per result, then the clocks rocm-smi reports"""
import argparse
import collections
import csv
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

SPACING = (2.5, 0.78125, 0.78125)
HBM_COPY_RATE = 6.29e12
# algorithmic bytes per voxel of the three passes of cf_edt: mask in, x offsets out; x offsets in, (x, y) offsets out; those in, fp64 out
PASS_BYTES = {"edt_x_kernel": 1 + 2, "edt_y_kernel": 2 + 4, "edt_z_kernel": 4 + 8}


def smi():
    try:
        o = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["rocm-smi unavailable: %s" % e]
    return [ln.strip() for ln in o.splitlines() if "GPU[0]" in ln and any(k in ln.lower() for k in ("sclk", "mclk", "power", "performance"))]


def ellipsoid_into(vol, label, centre, radii):
    import numpy as np
    lo = [max(0, int(c - r) - 1) for c, r in zip(centre, radii)]
    hi = [min(s, int(c + r) + 2) for c, r, s in zip(centre, radii, vol.shape)]
    g = np.indices([h - l for l, h in zip(lo, hi)]).astype(np.float64)
    inside = sum(((g[i] + lo[i] - centre[i]) / radii[i]) ** 2 for i in range(3)) <= 1.0
    sub = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    sub[inside] = label


def case(shape):
    """five organs placed as fractions of the volume: a liver-sized one down to a small one; test = shifted and rescaled"""
    import numpy as np
    D, H, W = shape
    organs = [((0.50, 0.34, 0.32), (0.30, 0.26, 0.24)), ((0.45, 0.70, 0.72), (0.20, 0.12, 0.14)), ((0.30, 0.72, 0.30), (0.12, 0.09, 0.10)),
              ((0.75, 0.66, 0.40), (0.10, 0.07, 0.06)), ((0.20, 0.30, 0.78), (0.06, 0.04, 0.04))]
    ref, test = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for k, (c, r) in enumerate(organs, 1):
        centre = [c[0] * D, c[1] * H, c[2] * W]
        radii = [r[0] * D, r[1] * H, r[2] * W]
        ellipsoid_into(ref, k, centre, radii)
        ellipsoid_into(test, k, [centre[0] + 1.0, centre[1] - 2.0, centre[2] + 3.0], [radii[0] * 0.96, radii[1] * 1.03, radii[2] * 0.98])
    return test, ref


def balls(r):
    import numpy as np
    side = 2 * r + 12
    g = np.indices((side,) * 3).astype(np.float64)
    a = sum((g[i] - (side / 2 - 1.5)) ** 2 for i in range(3)) <= r * r
    b = sum((g[i] - (side / 2 + 1.5)) ** 2 for i in range(3)) <= r * r
    return a, b


class Counting:
    """the ctypes library with every cf_* call counted by name"""

    def __init__(self, inner):
        self.inner, self.calls = inner, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not name.startswith("cf_") or name in ("cf_last_error", "cf_version", "cf_edt_workspace_bytes"):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def sample(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def alternate(fa, fb, runs):
    """-> (last results, samples of fa, samples of fb) [s]: one warm-up pair, then `runs` pairs, a then b"""
    ta, tb = [], []
    for i in range(runs + 1):
        ra, sa = sample(fa)
        rb, sb = sample(fb)
        if i:
            ta.append(sa)
            tb.append(sb)
    return ra, rb, ta, tb


def ms(ts):
    return [round(t * 1e3, 3) for t in ts]


def bench_case(shape, runs):
    import numpy as np
    from cineflow import evaluation, metrics
    from cineflow.evaluation import Evaluator
    test, ref = case(shape)
    labels = [1, 2, 3, 4, 5]
    ev = lambda route: Evaluator(labels=labels).evaluate(test, ref, advanced=True, voxel_spacing=SPACING, surface=route)       # noqa: E731
    ra, rb, ta, tb = alternate(lambda: ev("edt"), lambda: ev("pairs"), runs)
    worst = 0.0
    for name in ra:
        for m, v in ra[name].items():
            w = rb[name][m]
            if isinstance(v, float) and w == w and w != 0:
                worst = max(worst, abs(v - w) / abs(w))
    real = metrics.lib()
    calls = {}
    for route in ("edt", "pairs"):
        proxy = Counting(real)
        metrics.lib = evaluation.lib = lambda: proxy            # noqa: E731
        try:
            ev(route)
        finally:
            metrics.lib = evaluation.lib = lambda: real         # noqa: E731
        calls[route] = dict(proxy.calls)
    table = metrics.label_surface_edt_table(test, ref, labels, SPACING)
    borders = {str(c): [table[c]["n_test"], table[c]["n_ref"]] for c in labels}
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(json.dumps({"workload": "%d x %d x %d, five ellipsoidal organs, spacing %s" % (shape + (SPACING,)), "voxels": int(np.prod(shape)),
                      "border_voxels_test_ref": borders, "edt_ms": round(ma * 1e3, 2), "edt_samples_ms": ms(ta), "pairs_ms": round(mb * 1e3, 2),
                      "pairs_samples_ms": ms(tb), "pairs_over_edt": round(mb / ma, 2), "edt_calls": calls["edt"], "pairs_calls": calls["pairs"],
                      "worst_relative_difference": worst,
                      "surface_metrics": {n: {m: ra[n][m] for m in Evaluator.default_advanced_metrics} for n in ra}}), flush=True)
    return test, ref


def bench_sweep(radii, runs):
    from cineflow import metrics
    points = []
    for r in radii:
        a, b = balls(r)
        hd = lambda method: metrics.hausdorff_distance(a, b, voxel_spacing=SPACING, method=method)             # noqa: E731
        ra, rb, ta, tb = alternate(lambda: hd("edt"), lambda: hd("pairs"), runs)
        assert ra == rb, (r, ra, rb)
        e = metrics.label_surface_edt_table(a.astype("uint8"), b.astype("uint8"), [1], SPACING)[1]
        p = {"radius": r, "box": a.shape[0], "na": e["n_test"], "nb": e["n_ref"], "na_x_nb": e["n_test"] * e["n_ref"], "edt_samples_ms": ms(ta),
             "pairs_samples_ms": ms(tb), "edt_wins_every_repeat": max(ta) < min(tb)}
        points.append(p)
        print(json.dumps(p), flush=True)
    first = None
    for i in range(len(points) - 1, -1, -1):
        if not points[i]["edt_wins_every_repeat"]:
            break
        first = points[i]
    const = None if first is None else 1 << max(0, math.ceil(math.log2(first["na_x_nb"])))
    print(json.dumps({"sweep_first_point_from_which_edt_always_wins": None if first is None else first["radius"], "na_x_nb": first and first["na_x_nb"],
                      "smallest_power_of_two_at_or_above": const, "EDT_AUTO_PAIRS_in_use": metrics.EDT_AUTO_PAIRS}), flush=True)


def run_passes(shape, n):
    import numpy as np
    import torch
    from cineflow import metrics
    test, ref = case(shape)
    from scipy.ndimage import binary_erosion
    border = (ref > 0) ^ binary_erosion(ref > 0)
    mask = torch.from_numpy(~border).cuda()
    for _ in range(n):
        out = metrics.distance_transform_edt(mask, sampling=SPACING)
    torch.cuda.synchronize()
    vox = int(np.prod(shape))
    print(json.dumps({"passes_run": n, "voxels": vox, "largest_distance": float(out.max()),
                      "bytes_per_call": {k: v * vox for k, v in PASS_BYTES.items()}}), flush=True)


def run_visit(shape, n):
    import torch
    from cineflow import metrics
    test, ref = (torch.from_numpy(v).cuda() for v in case(shape))
    for _ in range(n):
        table = metrics.label_surface_edt_table(test, ref, [1, 2, 3, 4, 5], SPACING)
    torch.cuda.synchronize()
    print(json.dumps({"visits_run": n, "labels": 5, "hd": [table[c]["hd"] for c in (1, 2, 3, 4, 5)]}), flush=True)


def read_stats(path, shape):
    """path: rocprofv3's kernel_stats.csv (Name, Calls, AverageNs), or the rocpd database ROCm 7.2 writes instead (its top_kernels view:
    name, total_calls, total_duration, average [us], percentage), or that view exported as CSV"""
    vox = shape[0] * shape[1] * shape[2]
    if path.endswith(".db"):
        import sqlite3
        cur = sqlite3.connect(path).execute("select * from top_kernels")
        cols = [d[0] for d in cur.description]
        rows = [dict(zip(cols, r)) for r in cur]
    else:
        with open(path) as f:
            rows = list(csv.DictReader(f))
    for row in rows:
        name = row.get("Name") or row.get("name") or ""
        for k, per in PASS_BYTES.items():
            if k in name:
                avg_ns = float(row["AverageNs"]) if "AverageNs" in row else float(row["average"]) * 1e3
                rate = per * vox / (avg_ns * 1e-9)
                print(json.dumps({"kernel": k, "calls": int(row.get("Calls") or row.get("total_calls")), "average_us": round(avg_ns * 1e-3, 1),
                                  "algorithmic_bytes": per * vox, "achieved_TB_per_s": round(rate * 1e-12, 3),
                                  "share_of_hbm_copy_rate": round(rate / HBM_COPY_RATE, 3)}), flush=True)
        if "edt_" in name and not any(k in name for k in PASS_BYTES):              # the visit's own kernels: time only
            avg_us = float(row["AverageNs"]) * 1e-3 if "AverageNs" in row else float(row["average"])
            print(json.dumps({"kernel": name.split("(")[0].split("::")[-1], "calls": int(row.get("Calls") or row.get("total_calls")),
                              "average_us": round(avg_us, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 20 x 48 x 48 case and three small radii: a rehearsal of the script, not a measurement")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-case", action="store_true")
    ap.add_argument("--passes", type=int, default=0, help="only run N cf_edt calls on the case's border mask (for a kernel trace)")
    ap.add_argument("--visit", type=int, default=0, help="only run N label_surface_edt_table calls on device-resident volumes (for a kernel trace)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a traced --passes run: print each pass's achieved bytes/s")
    a = ap.parse_args()
    shape = (20, 48, 48) if a.small else (160, 384, 384)
    if a.stats:
        return read_stats(a.stats, shape)
    import torch
    assert torch.cuda.is_available(), "edt_bench needs a GPU"
    if a.passes:
        return run_passes(shape, a.passes)
    if a.visit:
        return run_visit(shape, a.visit)
    print(json.dumps({"clocks_before": smi()}), flush=True)
    if not a.no_case:
        bench_case(shape, a.runs)
    if not a.no_sweep:
        bench_sweep((3, 4, 6) if a.small else (3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96), a.runs)
    print(json.dumps({"clocks_after": smi()}), flush=True)


if __name__ == "__main__":
    main()
