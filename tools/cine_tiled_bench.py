"""Timing of the cine-batched sliding window (cineflow.inference.predict_cine_2Dconv_tiled) against the per-frame loop over
predict_3D_2Dconv_tiled, the chunk-size sweep behind TILE_JOBS_PER_LAUNCH and the peak device memory of a five-fold ensemble.

Workloads (BASELINE config 1 at its stated size, as a 30-frame cine): 30 volumes [1,10,256,216], patch (256,224) -> one tile per
slice; and 30 volumes [1,10,300,260], where the window slides (2 x 2 tiles per slice, Gaussian).  Generic_UNet(1, 32, 4, 6) with the
plan's (2,1) last pooling, seeded weights, 4 flips.  Both routes take host numpy volumes and return host numpy results.

    python tools/cine_tiled_bench.py                 every step below, each as a child process under its own time limit
    python tools/cine_tiled_bench.py --step timing   batched vs per-frame loop, same process, alternating: 2 warm-ups, median of 5
    python tools/cine_tiled_bench.py --step sweep    CF_TILE_JOBS-equivalent max_batch in 16 .. 512
    python tools/cine_tiled_bench.py --step memory   torch.cuda.max_memory_allocated, one fold vs five folds resident

Every step prints one JSON line per result."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

PATCH = (256, 224)
WORKLOADS = {"fov_256x216": (256, 216), "fov_300x260": (300, 260)}
STEP_LIMIT_S = {"timing": 420, "sweep": 420, "memory": 240}


def _net(seed, dev):
    from cineflow.models import Generic_UNet
    from cineflow.weights import seeded_state_dict
    net = Generic_UNet(1, 32, 4, 6, pool_op_kernel_sizes=[[2, 2]] * 5 + [[2, 1]])
    net.load_state_dict(seeded_state_dict(net.state_shapes(), seed), dev)
    return net


def _frames(shape, frames, slices, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    return [rng.randn(1, slices, shape[0], shape[1]).astype(np.float32) for _ in range(frames)]


def _timed(fn, warmup, runs):
    import torch
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return times


def step_timing(a):
    import torch
    from cineflow.inference import TILE_JOBS_PER_LAUNCH, predict_3D_2Dconv_tiled, predict_cine_2Dconv_tiled
    dev = torch.device("cuda:0")
    net = _net(41, dev)
    kw = dict(step_size=0.5, do_mirroring=True, mirror_axes=(0, 1), use_gaussian=True)
    for name, shape in WORKLOADS.items():
        vols = _frames(shape, a.frames, a.slices, 7)
        run_loop = lambda: [predict_3D_2Dconv_tiled(net, v, PATCH, **kw) for v in vols]          # noqa: E731
        run_batched = lambda: predict_cine_2Dconv_tiled(net, vols, PATCH, **kw)                    # noqa: E731
        _timed(run_loop, a.warmup, 0)
        _timed(run_batched, a.warmup, 0)
        loop, batched = [], []
        for _ in range(a.runs):                                                                     # the two routes alternate: drift hits both
            loop += _timed(run_loop, 0, 1)
            batched += _timed(run_batched, 0, 1)
        ml, mb = statistics.median(loop), statistics.median(batched)
        print(json.dumps({"step": "timing", "workload": name, "frames": a.frames, "slices": a.slices, "patch": PATCH, "chunk": TILE_JOBS_PER_LAUNCH,
                          "per_frame_loop_s": [round(t, 4) for t in loop], "batched_s": [round(t, 4) for t in batched],
                          "per_frame_loop_median_s": round(ml, 4), "batched_median_s": round(mb, 4), "batched_over_loop": round(mb / ml, 4)}), flush=True)


def step_sweep(a):
    import torch
    from cineflow.inference import predict_cine_2Dconv_tiled
    dev = torch.device("cuda:0")
    net = _net(41, dev)
    kw = dict(step_size=0.5, do_mirroring=True, mirror_axes=(0, 1), use_gaussian=True)
    for name, shape in WORKLOADS.items():
        vols = _frames(shape, a.frames, a.slices, 7)
        for chunk in (16, 32, 64, 128, 256, 512):
            torch.cuda.reset_peak_memory_stats()
            t = _timed(lambda: predict_cine_2Dconv_tiled(net, vols, PATCH, max_batch=chunk, **kw), 1, 3)
            print(json.dumps({"step": "sweep", "workload": name, "chunk": chunk, "median_s": round(statistics.median(t), 4),
                              "runs_s": [round(v, 4) for v in t], "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}), flush=True)


def step_memory(a):
    import torch
    from cineflow.inference import TILE_JOBS_PER_LAUNCH, predict_cine_2Dconv_tiled
    dev = torch.device("cuda:0")
    kw = dict(step_size=0.5, do_mirroring=True, mirror_axes=(0, 1), use_gaussian=True)
    vols = _frames(WORKLOADS["fov_256x216"], a.frames, a.slices, 7)
    nets = []
    for folds in (1, 5):
        while len(nets) < folds:
            nets.append(_net(41 + len(nets), dev))
        predict_cine_2Dconv_tiled(nets, vols, PATCH, **kw)                      # the packed weight forms are derived on first use
        torch.cuda.synchronize()
        weights = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t = _timed(lambda: predict_cine_2Dconv_tiled(nets, vols, PATCH, **kw), 0, 1)
        print(json.dumps({"step": "memory", "folds": folds, "workload": "fov_256x216", "frames": a.frames, "slices": a.slices,
                          "chunk": TILE_JOBS_PER_LAUNCH, "resident_before_GiB": round(weights / 2 ** 30, 3),
                          "max_memory_allocated_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "run_s": round(t[0], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--slices", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.step is not None:
        return {"timing": step_timing, "sweep": step_sweep, "memory": step_memory}[a.step](a)
    # every GPU step is a fresh child under a time limit of its own; the first one that fails or overruns ends the run
    for step in ("timing", "sweep", "memory"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--frames", str(a.frames),
               "--slices", str(a.slices), "--warmup", str(a.warmup), "--runs", str(a.runs)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
