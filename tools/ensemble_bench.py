"""Merging saved softmax folders (cineflow.ensemble_predictions): where a case's time goes.

Workloads: a cardiac-sized case (K = 4, crop (10, 256, 216) at (0, 2, 4) in (10, 260, 224)) and a 3d_fullres-sized one (K = 4, crop
(96, 224, 224) at (2, 4, 8) in (100, 232, 240)), fp16 members, N = 2 and 5.  Members are seeded softmaxes of blocky logits (coarse
8 N(0,1) noise repeated over 4 x 16 x 16 voxels plus 0.5 N(0,1) per voxel): large confident regions with noisy borders, so that the .npz
files compress roughly as a network's do -- a softmax of white noise would not compress at all.

    (a) kernel      cf_ensemble_merge alone on device-resident members, by device events, without and with the mean output; GB/s from the
                    bytes it must move: N x K x voxels x 2 read, the label volume written, K x voxels x 2 more with the mean
    (b) merge_files per-case wall time split into load (np.load + inflate + properties) / device (host-to-device copies, the kernel,
                    the labels coming back) / write (.nii.gz), from ensemble_predictions.LAST_TIMING; medians over --runs calls after a warm-up
    (c) numpy       the same loaded arrays through np.mean(np.vstack(...), 0), argmax(0) and the bounding-box placement on the host

    python tools/ensemble_bench.py [--calls 20] [--runs 5] [--small]       one JSON line per (workload, N), then the clocks rocm-smi reports"""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

# name: (K, crop, volume, where the crop goes)
WORKLOADS = {"cardiac_10x256x216": (4, (10, 256, 216), (10, 260, 224), (0, 2, 4)),
             "fullres_96x224x224": (4, (96, 224, 224), (100, 232, 240), (2, 4, 8))}
SMALL = {"small_3x40x36": (4, (3, 40, 36), (4, 44, 40), (0, 2, 3))}          # --small: a rehearsal of the script, not a measurement
MEMBERS = (2, 5)
HBM_COPY_TBS = 6.29          # measured float4 copy rate of an MI355X (8.0 TB/s specified)


def smi():
    try:
        o = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["rocm-smi unavailable: %s" % e]
    return [ln.strip() for ln in o.splitlines() if "GPU[0]" in ln and any(k in ln.lower() for k in ("sclk", "mclk", "power", "performance"))]


def blocky_softmax(K, crop, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    coarse = rng.standard_normal((K,) + tuple((n + b - 1) // b for n, b in zip(crop, (4, 16, 16))), dtype=np.float32)
    logits = 8 * coarse.repeat(4, 1).repeat(16, 2).repeat(16, 3)[:, :crop[0], :crop[1], :crop[2]]
    logits = logits + 0.5 * rng.standard_normal((K,) + tuple(crop), dtype=np.float32)
    e = np.exp(logits - logits.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(np.float16)


def numpy_merge(members, full, lo):
    import numpy as np
    mean = np.mean(np.vstack([a[None] for a in members]), 0)
    seg = mean.argmax(0)
    out = np.zeros(full, dtype=np.uint8)
    out[tuple(slice(a, a + n) for a, n in zip(lo, seg.shape))] = seg
    return out, mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "ensemble_bench needs a GPU"
    from cineflow import ensemble_predictions as E
    from cineflow import ops
    from cineflow.nifti import read_nifti
    dev = torch.device("cuda:0")
    print(json.dumps({"clocks_before": smi()}), flush=True)
    for name, (K, crop, full, lo) in (SMALL if a.small else WORKLOADS).items():
        voxels = crop[0] * crop[1] * crop[2]
        all_members = [blocky_softmax(K, crop, 40 + i) for i in range(max(MEMBERS))]
        with tempfile.TemporaryDirectory() as tmp:
            props = {"size_after_cropping": tuple(crop), "original_size_of_raw_data": np.array(full),
                     "crop_bbox": [[s, s + n] for s, n in zip(lo, crop)], "itk_spacing": (1.5, 1.5, 8.0), "itk_origin": (0.0, 0.0, 0.0),
                     "itk_direction": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}
            for i, m in enumerate(all_members):
                os.makedirs(os.path.join(tmp, "m%d" % i))
                np.savez_compressed(os.path.join(tmp, "m%d" % i, "case.npz"), softmax=m)
                with open(os.path.join(tmp, "m%d" % i, "case.pkl"), "wb") as f:
                    pickle.dump(props, f)
            npz_bytes = [os.path.getsize(os.path.join(tmp, "m%d" % i, "case.npz")) for i in range(len(all_members))]
            for N in MEMBERS:
                members = all_members[:N]
                # (c) the host statement, on arrays already in memory
                tc = []
                for _ in range(max(2, a.runs // 2)):
                    t0 = time.perf_counter()
                    want_seg, want_mean = numpy_merge(members, full, lo)
                    tc.append(time.perf_counter() - t0)
                # (a) the kernel alone
                on_dev = [torch.from_numpy(m).to(dev) for m in members]
                seg = torch.empty(full, dtype=torch.uint8, device=dev)
                mean = torch.empty_like(on_dev[0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                kernel = {}
                for tag, mean_out in (("labels_only", None), ("with_mean", mean)):
                    tk = []
                    for _ in range(a.runs + 1):                                   # the first sample is the warm-up
                        e0.record()
                        for _ in range(a.calls):
                            ops._ensemble_merge_into(on_dev, seg, lo, mean_out, None)
                        e1.record()
                        e1.synchronize()
                        tk.append(e0.elapsed_time(e1) * 1e-3 / a.calls)
                    mk = statistics.median(tk[1:])
                    nbytes = N * K * voxels * 2 + full[0] * full[1] * full[2] + (K * voxels * 2 if mean_out is not None else 0)
                    kernel[tag] = {"median_us": round(mk * 1e6, 1), "samples_us": [round(t * 1e6, 1) for t in tk[1:]], "bytes": nbytes,
                                   "GBs": round(nbytes / mk / 1e9, 1), "share_of_hbm_copy_rate": round(nbytes / mk / (HBM_COPY_TBS * 1e12), 4)}
                same = bool(np.array_equal(seg.cpu().numpy(), want_seg)) and bool(np.array_equal(mean.cpu().numpy().view(np.uint16), want_mean.view(np.uint16)))
                del on_dev
                # (b) the file-level call
                files = [os.path.join(tmp, "m%d" % i, "case.npz") for i in range(N)]
                pkls = [f[:-4] + ".pkl" for f in files]
                out_file = os.path.join(tmp, "out_%d.nii.gz" % N)
                split = {"load_s": [], "device_s": [], "write_s": []}
                for r in range(a.runs + 1):
                    E.merge_files(files, pkls, out_file, True, False)
                    if r:
                        for k in split:
                            split[k].append(E.LAST_TIMING[k])
                same_file = bool(np.array_equal(read_nifti(out_file)[0], want_seg))
                med = {k: statistics.median(v) for k, v in split.items()}
                print(json.dumps({"workload": name, "N": N, "K": K, "crop": crop, "volume": full, "npz_MB": round(sum(npz_bytes[:N]) / 1e6, 2),
                                  "raw_MB": round(N * K * voxels * 2 / 1e6, 2), "kernel": kernel, "kernel_equals_numpy": same,
                                  "merge_files_ms": {k: round(v * 1e3, 2) for k, v in med.items()},
                                  "merge_files_total_ms": round(sum(med.values()) * 1e3, 2),
                                  "merge_files_samples_ms": {k: [round(t * 1e3, 2) for t in v] for k, v in split.items()},
                                  "file_equals_numpy": same_file, "numpy_host_ms": round(statistics.median(tc) * 1e3, 2),
                                  "numpy_host_samples_ms": [round(t * 1e3, 2) for t in tc]}), flush=True)
    print(json.dumps({"clocks_after": smi()}), flush=True)


if __name__ == "__main__":
    main()
