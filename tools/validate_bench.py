"""The export of one validated case: the one-visit kernel against the composed route it replaces in cineflow.validate.

Both routes start from the case's softmax as a device tensor [K, *stage shape] (file axis order) and end with the same three host results:
the uint8 label volume at the size before cropping, the stored fp16 softmax at the size after cropping, and the 16 x 16 label confusion
against the ground truth (resident on the device for both).

    (a) fused     one ops.resample_argmax call (cf_resample_argmax) and the read-back of its three outputs
    (b) composed  the parent commit's functions: softmax to the host, ops.resample_data_or_seg (upload, cf_resize3d, K fp32 volumes back),
                  numpy arg-max and placement, export.probabilities_as_stored, then metrics.label_histogram on the uploaded labels

Workloads, K = 4, seeded blocky softmaxes (tools/ensemble_bench.py's):
    cine     a short-axis cine case resampled in plane only: stage (246, 292, 10) -> crop (216, 256, 10) at (4, 2, 0) in (224, 260, 10),
             linear in plane, nearest along the slice axis (the separate-z case)
    fullres  a 3d_fullres-like case: stage (192, 192, 80) -> crop (224, 224, 96) at (4, 8, 2) in (232, 240, 100), linear on every axis

A sample is the wall time of one case (device synchronised before and after); the routes alternate and take turns to go first, `--runs`
samples each after one warm-up round; medians and every sample are printed.  The results of the two routes are compared before timing.

--compress adds a second line per workload: the case's FILES (validation_raw's <case>.nii.gz, .npz and .pkl) written by the default
route (read back, np.savez_compressed at zlib level 6 and the .nii.gz at level 2, on the calling thread) against compress="device"
(cf_deflate + cf_crc32 on the tensors, compressed bytes read back, containers written by hand), alternating like the routes above; wall
time of one case on one thread, and the bytes of the files.

    python tools/validate_bench.py [--runs 7] [--small] [--compress]      JSON lines per workload, between the clocks rocm-smi reports"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K = 4
HIST_K = 16
# name: (stage shape, crop, full volume, where the crop goes, linear flags)
WORKLOADS = {"cine": ((246, 292, 10), (216, 256, 10), (224, 260, 10), (4, 2, 0), (1, 1, 0)),
             "fullres": ((192, 192, 80), (224, 224, 96), (232, 240, 100), (4, 8, 2), (1, 1, 1))}
SMALL = {"small": ((22, 26, 5), (19, 23, 5), (21, 24, 6), (1, 0, 1), (1, 1, 0))}          # --small: a rehearsal of the script, not a measurement


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--compress", action="store_true", help="also time the case's files under both compress settings")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "validate_bench needs a GPU"
    from cineflow import export, metrics, ops
    from ensemble_bench import blocky_softmax, smi
    dev = torch.device("cuda:0")
    print(json.dumps({"clocks_before": smi()}), flush=True)
    for name, (stage, crop, full, lo, lin) in (SMALL if a.small else WORKLOADS).items():
        softmax = torch.from_numpy(blocky_softmax(K, stage, 71).astype(np.float32)).to(dev)     # the network's softmax is fp32
        gt = torch.from_numpy(blocky_softmax(K, full, 72).argmax(0).astype(np.uint8)).to(dev)
        separate = [i for i, l in enumerate(lin) if not l]
        box = tuple(slice(o, o + n) for o, n in zip(lo, crop))

        def fused():
            seg, probs, hist = ops.resample_argmax(softmax, crop, lin, full_shape=full, bbox_lo=lo, want_probs=True, gt=gt)
            return seg.cpu().numpy(), probs.cpu().numpy(), hist.cpu().numpy()

        def composed():
            host = softmax.cpu().numpy()
            res = ops.resample_data_or_seg(host, crop, False, axis=separate or None, order=1, do_separate_z=bool(separate), order_z=0)
            seg = np.zeros(full, dtype=np.uint8)
            seg[box] = res.argmax(0)
            stored = export.probabilities_as_stored(res)
            hist, overflow = metrics.label_histogram(torch.from_numpy(seg).to(dev), gt, HIST_K)
            return seg, stored, np.concatenate([hist.reshape(-1), [overflow]])

        ra, rb = fused(), composed()
        equal = all(np.array_equal(x, y) for x, y in zip(ra, rb))

        def sample(route):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            route()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        ta, tb = [], []
        for r in range(a.runs + 1):                                                   # the first round is the warm-up
            first, second = (fused, composed) if r % 2 == 0 else (composed, fused)     # alternate, and alternate who goes first
            x, y = sample(first), sample(second)
            if r:
                ta.append(x if first is fused else y)
                tb.append(y if first is fused else x)
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps({"workload": name, "K": K, "stage": stage, "crop": crop, "full": full, "linear": lin, "results_equal": bool(equal),
                          "fused_ms": round(ma * 1e3, 3), "fused_samples_ms": [round(t * 1e3, 3) for t in ta],
                          "composed_ms": round(mb * 1e3, 3), "composed_samples_ms": [round(t * 1e3, 3) for t in tb],
                          "composed_over_fused": round(mb / ma, 2)}), flush=True)
        if a.compress:
            import tempfile
            from cineflow import validate as V
            from cineflow.nifti import read_nifti
            props = {"itk_spacing": (1.4, 1.4, 10.0), "itk_origin": (0.0, 0.0, 0.0), "itk_direction": (1, 0, 0, 0, 1, 0, 0, 0, 1)}
            with tempfile.TemporaryDirectory(prefix="valbench_") as tmp:
                files = {c: os.path.join(tmp, c + ".nii.gz") for c in ("zlib", "device")}

                def write_zlib():
                    seg, probs, _hist = fused()
                    V._write_case(files["zlib"], seg, probs, dict(props), None)

                def write_device():
                    seg, probs, hist = ops.resample_argmax(softmax, crop, lin, full_shape=full, bbox_lo=lo, want_probs=True, gt=gt)
                    hist.cpu()
                    packed = V._pack_case(files["device"], seg, probs, props)
                    V._write_case(files["device"], packed[0], packed[1], dict(props), None, "device")

                tz, td = [], []
                for r in range(a.runs + 1):
                    first, second = (write_zlib, write_device) if r % 2 == 0 else (write_device, write_zlib)
                    x, y = sample(first), sample(second)
                    if r:
                        tz.append(x if first is write_zlib else y)
                        td.append(y if first is write_zlib else x)
                same = np.array_equal(read_nifti(files["zlib"])[0], read_nifti(files["device"])[0]) and \
                    np.array_equal(np.load(files["zlib"][:-7] + ".npz")["softmax"], np.load(files["device"][:-7] + ".npz")["softmax"])
                size = {c: {e: os.path.getsize(f[:-7] + e) for e in (".nii.gz", ".npz")} for c, f in files.items()}
            print(json.dumps({"workload": name, "files": True, "contents_equal": bool(same), "zlib_ms": round(statistics.median(tz) * 1e3, 3),
                              "zlib_samples_ms": [round(t * 1e3, 3) for t in tz], "device_ms": round(statistics.median(td) * 1e3, 3),
                              "device_samples_ms": [round(t * 1e3, 3) for t in td], "zlib_over_device": round(statistics.median(tz) / statistics.median(td), 2),
                              "file_bytes": size}), flush=True)
    print(json.dumps({"clocks_after": smi()}), flush=True)


if __name__ == "__main__":
    main()
