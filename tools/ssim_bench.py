"""SSIM of a registered cine (cineflow.metrics.cine_ssim_table): one visit per patient against the per-pair path it replaces.

Workload: one synthetic patient of 30 frames x 10 slices x 256 x 256, three structures (an LV disc inside a MYO ring beside an RV disc),
images N(300, 40^2) with per-frame noise, smooth flows of amplitude 1.6; every array starts in host memory, as cineflow.score has them
after reading the files.

    (a) table   metrics.cine_ssim_table(fixed, moving, flow, labels): one cf_warp_bilinear_2d (B = T D), one cf_cine_ssim_table, one read
    (b) loop    per (frame, slice): ops.warp_bilinear, data_range = max - min of the registered slice, metrics.structural_similarity(full=True)
                and the three `ssim_img[seg == k].mean()` on the host -- the path that existed before the table
    (c) kernel  cf_cine_ssim_table alone on device-resident arrays, by device events

Wall times are synchronised medians of --runs calls after a warm-up; the library calls of one (a) and one (b) are counted by name.

    python tools/ssim_bench.py [--runs 7] [--calls 20] [--small]           one JSON line, then the clocks rocm-smi reports"""
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

NAMES = ("RV", "MYO", "LV")


def smi():
    try:
        o = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["rocm-smi unavailable: %s" % e]
    return [ln.strip() for ln in o.splitlines() if "GPU[0]" in ln and any(k in ln.lower() for k in ("sclk", "mclk", "power", "performance"))]


def patient(T, D, H, W, seed=3):
    import numpy as np
    rng = np.random.default_rng(seed)
    fixed = rng.normal(300.0, 40.0, size=(H, W, D))
    moving = (fixed[None] + rng.normal(0.0, 10.0, size=(T, H, W, D))).astype(np.float32)
    flow = rng.normal(size=(T, H, W, D, 2))
    for ax in (1, 2):
        flow = (np.roll(flow, 1, ax) + flow + np.roll(flow, -1, ax)) / 3.0
    flow = (flow * 1.6).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    labels = np.zeros((H, W, D), np.uint8)
    for d in range(D):
        r = np.hypot(yy - H / 2, xx - W / 2 - W / 16)
        r1 = H / 10 + d % 3
        labels[:, :, d][np.hypot(yy - H / 2, xx - W / 2 + W / 5) <= H / 12] = 1
        labels[:, :, d][r <= r1 + H / 24] = 2
        labels[:, :, d][r <= r1] = 3
    return fixed, moving, flow, labels


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


def per_pair_loop(fixed, moving, flow, labels, win):
    """the rows of cine_ssim_table from one call chain per (frame, slice)"""
    import numpy as np
    import torch
    from cineflow import metrics, ops
    dev = torch.device("cuda:0")
    T, H, W, D = moving.shape
    rows = []
    for d in range(D):
        for t in range(T):
            f = torch.from_numpy(np.ascontiguousarray(flow[t, :, :, d].transpose(2, 0, 1)))[None].to(dev)
            m = torch.from_numpy(np.ascontiguousarray(moving[t, :, :, d]))[None, None].to(dev)
            reg = ops.warp_bilinear(f, m)[0, 0].cpu().numpy()
            score, smap = metrics.structural_similarity(fixed[:, :, d], reg, win_size=win, data_range=reg.max() - reg.min(), full=True)
            per = [float(smap[labels[:, :, d] == k].mean()) for k in (1, 2, 3)]
            row = {"SSIM_whole": score, "SSIM_mean": sum(per) / 3}
            row.update({"SSIM_" + n.lower(): v for n, v in zip(NAMES, per)})
            rows.append(row)
    return rows


def timed(fn, runs):
    import torch
    out = []
    for _ in range(runs + 1):                                                  # the first sample is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return res, out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--win", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="3 frames x 2 slices x 64 x 64: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "ssim_bench needs a GPU"
    from cineflow import _lib, metrics
    T, D, H, W = (3, 2, 64, 64) if a.small else (30, 10, 256, 256)
    fixed, moving, flow, labels = patient(T, D, H, W)
    print(json.dumps({"clocks_before": smi()}), flush=True)

    table = lambda: metrics.cine_ssim_table(fixed, moving, flow, labels, NAMES, a.win)                    # noqa: E731
    loop = lambda: per_pair_loop(fixed, moving, flow, labels, a.win)                                      # noqa: E731
    rows_a, ta = timed(table, a.runs)
    rows_b, tb = timed(loop, a.runs)
    worst = max(abs(ra[k] - rb[k]) for ra, rb in zip(rows_a, rows_b) for k in ra)

    real = _lib.lib()
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

    # (c) the three launches alone
    dev = torch.device("cuda:0")
    _, reg = metrics.ssim_sums_table(fixed, moving, flow, labels, 4, a.win)
    fx = torch.from_numpy(fixed).to(dev).permute(2, 0, 1).contiguous()
    lab = torch.from_numpy(labels).to(dev).permute(2, 0, 1).contiguous()
    cols = 2 + 2 * 4
    rng = torch.empty(T * D * 2, dtype=torch.float32, device=dev)
    part = torch.empty(T * D * (-(-H // 32)) * (-(-W // 64)) * cols, dtype=torch.float64, device=dev)
    out = torch.empty(T * D * cols, dtype=torch.float64, device=dev)
    NP = a.win * a.win
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tk = []
    for _ in range(a.runs + 1):
        e0.record()
        for _ in range(a.calls):
            _lib.check(real.cf_cine_ssim_table(fx.data_ptr(), reg.data_ptr(), lab.data_ptr(), T, D, H, W, 4, a.win, 0.01, 0.03, NP / (NP - 1.0),
                                               rng.data_ptr(), part.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream), "cf_cine_ssim_table")
        e1.record()
        e1.synchronize()
        tk.append(e0.elapsed_time(e1) * 1e-3 / a.calls)
    ma, mb, mk = statistics.median(ta), statistics.median(tb), statistics.median(tk[1:])
    print(json.dumps({"workload": "%d frames x %d slices x %d x %d, win %d" % (T, D, H, W, a.win), "pixels": T * D * H * W,
                      "table_ms": round(ma * 1e3, 2), "table_samples_ms": [round(t * 1e3, 2) for t in ta],
                      "loop_ms": round(mb * 1e3, 2), "loop_samples_ms": [round(t * 1e3, 2) for t in tb],
                      "loop_over_table": round(mb / ma, 2), "table_calls": calls_a, "loop_calls": calls_b,
                      "kernel_us": round(mk * 1e6, 1), "kernel_samples_us": [round(t * 1e6, 1) for t in tk[1:]],
                      "kernel_Mpixel_per_s": round(T * D * H * W / mk / 1e6, 1), "worst_difference": float(worst)}), flush=True)
    print(json.dumps({"clocks_after": smi()}), flush=True)
    assert np.isfinite(worst) and worst <= 1e-9, worst


if __name__ == "__main__":
    main()
