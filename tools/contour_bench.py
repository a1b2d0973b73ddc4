"""Contour tracking of a patient (cineflow.strain.track_patient): one visit per patient against the per-slice, per-step path it replaces.

Workload: one synthetic patient of 30 frames x 10 slices x 256 x 256 with 3 x 80 contour points per slice (endo and epi rings and an RV
ring, contracting and relaxing over the cine, with 0.2 px of noise), smooth flows of amplitude 1.6 px; every array starts in host
memory, as cineflow.score has them after reading the files.  For each of the four modes of nnunet/compute_contour_metrics.py:

    (a) patient  strain.track_patient(flow, pts, counts, mode): one upload, one cf_contour_track_table (and one cf_contour_strain_table
                 in mode from_ed, which also returns the strain curves), one read
    (b) loop     per slice strain.contour_tracking_error(flow[d], pts[d], split, mode) (and strain.from_ed in mode from_ed): one
                 cf_sample_points_2d per chain step, the flow frame uploaded and the points read back every time
    (c) kernel   cf_contour_track_table alone on device-resident arrays, by device events

Wall times are synchronised medians of --runs calls after a warm-up, (a) and (b) sampled alternately; the library calls of one (a) and one
(b) are counted by name.  The kernel walks chains of dependent gathers: its time is reported as it is, against no peak.

    python tools/contour_bench.py [--runs 5] [--calls 20] [--small]           one JSON line per mode, then the clocks rocm-smi reports"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

MODES = ("from_ed", "from_ed_accumulation", "to_ed_accumulation", "to_ed")
ZOOM = (1.25, 1.25)


def smi():
    try:
        o = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["rocm-smi unavailable: %s" % e]
    return [ln.strip() for ln in o.splitlines() if "GPU[0]" in ln and any(k in ln.lower() for k in ("sclk", "mclk", "power", "performance"))]


def patient(T, D, A, B, P, seed=5):
    """-> flow fp32 [D, T, 2, A, B] with frame 0 NaN (strain.prepare_flow's layout), pts fp32 [D, T, 3 P, 2], counts int32 [D, 3]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    flow = rng.normal(size=(D, T, 2, A, B))
    for ax in (3, 4):
        flow = (np.roll(flow, 1, ax) + flow + np.roll(flow, -1, ax)) / 3.0
    flow = (flow * 1.6).astype(np.float32)
    flow[:, 0] = np.nan
    ang = np.linspace(0, 2 * np.pi, P, endpoint=False)
    pts = np.zeros((D, T, 3 * P, 2), np.float32)
    for d in range(D):
        for t in range(T):
            k = 1.0 - 0.15 * np.sin(np.pi * t / T)
            for j, (r, cx) in enumerate(((0.12, 0.55), (0.18, 0.55), (0.10, 0.25))):
                ring = np.stack([B * (cx + r * k * np.cos(ang)), A * (0.5 + r * k * np.sin(ang))], axis=-1) + rng.normal(0, 0.2, (P, 2))
                pts[d, t, j * P:(j + 1) * P] = ring
    return flow, pts, np.full((D, 3), P, np.int32)


class Counting:
    """the ctypes library with every cf_* call counted by name"""

    def __init__(self, inner):
        self.inner, self.calls = inner, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not name.startswith("cf_") or name in ("cf_last_error", "cf_version"):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def per_slice_loop(flow, pts, counts, mode):
    """the numbers of track_patient from the per-launch functions, slice by slice"""
    import numpy as np
    from cineflow import strain
    errors, curves = [], []
    for d in range(len(flow)):
        c = counts[d]
        errors.append(strain.contour_tracking_error(flow[d], pts[d], np.cumsum(c[:2]), mode))
        if mode == "from_ed":
            r = strain.from_ed(flow[d], np.stack([pts[d, :, :c[0]], pts[d, :, c[0]:2 * c[0]]]), ZOOM)
            curves.append(np.stack([r["radial_strain"].numpy(), r["circ_strain"].numpy()], axis=-1))
    return np.stack(errors), (np.stack(curves) if curves else None)


def sample(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="4 frames x 2 slices x 32 x 32, 3 x 8 points: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "contour_bench needs a GPU"
    from cineflow import _lib, metrics, strain
    T, D, A, B, P = (4, 2, 32, 32, 8) if a.small else (30, 10, 256, 256, 80)
    flow, pts, counts = patient(T, D, A, B, P)
    print(json.dumps({"clocks_before": smi()}), flush=True)
    dev = torch.device("cuda:0")
    real = _lib.lib()
    missed = []
    for mode in MODES:
        zoom = ZOOM if mode == "from_ed" else None
        table = lambda: strain.track_patient(flow, pts, counts, mode, zoom)                             # noqa: E731
        loop = lambda: per_slice_loop(flow, pts, counts, mode)                                          # noqa: E731
        ta, tb = [], []
        for i in range(a.runs + 1):                                                                      # the first pair is the warm-up
            res_a, sa = sample(table)
            res_b, sb = sample(loop)
            if i:
                ta.append(sa)
                tb.append(sb)
        worst = float(np.abs(res_a["errors"] - res_b[0]).max())
        worst_strain = float(np.abs(res_a["strain"] - res_b[1]).max()) if zoom else None

        proxy = Counting(real)
        _lib._lib = proxy
        try:
            table()
            calls_a = dict(proxy.calls)
            proxy.calls.clear()
            loop()
            calls_b = dict(proxy.calls)
        finally:
            _lib._lib = real

        # (c) the two launches of cf_contour_track_table alone
        f, p = torch.from_numpy(flow).to(dev), torch.from_numpy(pts).to(dev)
        cd = torch.from_numpy(counts).to(dev)
        pos = torch.empty((D, T - 1, 3 * P, 2), dtype=torch.float32, device=dev)
        out = torch.empty(D * (T - 1) * 3, dtype=torch.float64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tk = []
        for _ in range(a.runs + 1):
            e0.record()
            for _ in range(a.calls):
                _lib.check(real.cf_contour_track_table(f.data_ptr(), p.data_ptr(), counts.ctypes.data, cd.data_ptr(), D, T, A, B, 3 * P,
                                                       metrics.CONTOUR_MODES.index(mode), pos.data_ptr(), out.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream), "cf_contour_track_table")
            e1.record()
            e1.synchronize()
            tk.append(e0.elapsed_time(e1) * 1e-3 / a.calls)
        ma, mb, mk = statistics.median(ta), statistics.median(tb), statistics.median(tk[1:])
        steps = D * 3 * P * {"from_ed": T - 1, "from_ed_accumulation": T - 1, "to_ed_accumulation": T * (T - 1) // 2, "to_ed": T - 1}[mode]
        print(json.dumps({"mode": mode, "workload": "%d frames x %d slices x %d x %d, 3 x %d points per slice" % (T, D, A, B, P),
                          "patient_ms": round(ma * 1e3, 2), "patient_samples_ms": [round(t * 1e3, 2) for t in ta],
                          "loop_ms": round(mb * 1e3, 2), "loop_samples_ms": [round(t * 1e3, 2) for t in tb],
                          "loop_over_patient": round(mb / ma, 2), "patient_calls": calls_a, "loop_calls": calls_b,
                          "kernel_us": round(mk * 1e6, 1), "kernel_samples_us": [round(t * 1e6, 1) for t in tk[1:]], "chain_steps": steps,
                          "worst_error_difference": worst, "worst_strain_difference": worst_strain}), flush=True)
        # the per-launch functions subtract coordinates in fp32 (tests/test_strain.py holds them to 1e-4 and 1e-5)
        if not (np.isfinite(worst) and worst <= 1e-4 and (worst_strain is None or worst_strain <= 1e-5)):
            missed.append((mode, worst, worst_strain))
    print(json.dumps({"clocks_after": smi()}), flush=True)
    assert not missed, missed


if __name__ == "__main__":
    main()
