"""Timing of MTLmodel as the segmentation network of a sliding-window batch: the device-resident batched wrapper
(MTLmodel.accumulate_tta_batch: one cropper forward at B, cf_crop_windows, one cf_tile_gather, one network call per flip at B,
cf_tta_accumulate_window) against the per-sample wrapper MTLmodel.mirror_and_predict_2d (per sample: cropper forward at B = 1, boxes
read back to the host, crop; then the flips at B and one ops.pad2d per sample) on the SAME device batch.

Full width (adversarial_acdc.yaml / seg_model.yaml), image 224, crop 128, B = 64 (inference.TILE_JOBS_PER_LAUNCH), 4 flips, seeded
weights, unit-scale structured input.  The cropper runs at window 7 (224, 112, 56 are multiples of 7); the segmenter on the 128 x 128 crop
runs at window 8: its skip maps are 128, 64 and 32 wide, which 7 does not divide -- the pair (crop 128, window 7) of
nnMTLTrainerV2.py:110-121 cannot be built (the reference's window_partition needs the division too, as cf_window_attention does).
Warm-up first, every sample synchronised before and after, the two paths sampled alternately (drift hits both), median of the samples.
One extra pass of each path runs with a counting proxy in front of the library handle: calls into libcineflow_hip.so per path, by
entry point.

    python tools/mtl_seg_bench.py [--batch 64] [--warmup 2] [--runs 7] [--markdown profiles/mtl_seg.md]

Prints one JSON line; --markdown also writes the samples and the call counts as a table."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

IMAGE, CROP, WINDOW, SEG_WINDOW, FLIPS = 224, 128, 7, 8, 4


class _Counting:
    """the library handle with every cf_* call counted by name"""

    def __init__(self, handle, counts):
        self._handle, self._counts = handle, counts

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.startswith("cf_"):
            return fn

        def call(*a):
            self._counts[name] += 1
            return fn(*a)
        return call


def _input(B, seed):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.randn(B, 1, 7, 7, generator=g), size=(IMAGE, IMAGE), mode="bicubic", align_corners=False)
    return x + 0.1 * torch.randn(B, 1, IMAGE, IMAGE, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    import torch
    from cineflow import _lib
    from cineflow.inference import Processor
    from cineflow.mtl import MTLmodel
    from cineflow.weights import seeded_state_dict
    dev = torch.device("cuda:0")
    crop = MTLmodel(IMAGE, WINDOW, 2)
    crop.load_state_dict(seeded_state_dict(crop.state_shapes(), 73), dev)
    seg = MTLmodel(CROP, SEG_WINDOW, 4, processor=Processor(CROP, IMAGE, crop))
    seg.load_state_dict(seeded_state_dict(seg.state_shapes(), 74), dev)
    x = _input(a.batch, 5).to(dev)

    def batched():
        acc = torch.zeros((a.batch, 4, IMAGE, IMAGE), dtype=torch.float32, device=dev)
        seg.accumulate_tta_batch(x, acc, 1.0 / FLIPS)
        return acc

    def per_sample():
        return seg.mirror_and_predict_2d(x)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(a.warmup):
        timed(per_sample)
        timed(batched)
    ts, tb = [], []
    for _ in range(a.runs):
        ts.append(timed(per_sample))
        tb.append(timed(batched))
    diff = float((batched() - per_sample()).abs().max())
    counts = {}
    real = _lib.lib()
    for name, fn in (("per_sample", per_sample), ("batched", batched)):
        counts[name] = collections.Counter()
        _lib._lib = _Counting(real, counts[name])
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            _lib._lib = real
    ms, mb = statistics.median(ts), statistics.median(tb)
    res = {"tool": "mtl_seg_bench", "image": IMAGE, "crop": CROP, "window": WINDOW, "segmenter_window": SEG_WINDOW, "batch": a.batch, "flips": FLIPS, "warmup": a.warmup,
           "per_sample_s": [round(t, 4) for t in ts], "batched_s": [round(t, 4) for t in tb], "per_sample_median_s": round(ms, 4),
           "batched_median_s": round(mb, 4), "batched_over_per_sample": round(mb / ms, 4), "max_abs_diff": diff,
           "library_calls": {k: sum(v.values()) for k, v in counts.items()}, "library_calls_by_name": {k: dict(sorted(v.items())) for k, v in counts.items()}}
    print(json.dumps(res), flush=True)
    if a.markdown:
        names = sorted(set(counts["per_sample"]) | set(counts["batched"]))
        with open(a.markdown, "w") as f:
            f.write("# MTLmodel as the segmentation network: batched wrapper against the per-sample wrapper\n\n")
            f.write("`python tools/mtl_seg_bench.py --batch %d --warmup %d --runs %d` on one MI355X.  Full width, image %d, crop %d, window %d (cropper) / %d "
                    "(segmenter: 7 does not divide its 128 / 64 / 32 maps), %d flips, B = %d; warm-up first, every sample synchronised, the two paths sampled alternately.\n\n"
                    % (a.batch, a.warmup, a.runs, IMAGE, CROP, WINDOW, SEG_WINDOW, FLIPS, a.batch))
            f.write("| path | samples [s] | median [s] |\n|---|---|---|\n")
            f.write("| per-sample wrapper (`MTLmodel.mirror_and_predict_2d`) | %s | %.4f |\n" % (", ".join("%.4f" % t for t in ts), ms))
            f.write("| batched wrapper (`MTLmodel.accumulate_tta_batch`) | %s | %.4f |\n\n" % (", ".join("%.4f" % t for t in tb), mb))
            f.write("Ratio batched / per-sample: **%.4f** (%s).  Largest difference between the two results: %.3e.\n\n"
                    % (mb / ms, "the batched path is faster" if mb < ms else "the batched path is NOT faster at this batch size", diff))
            f.write("Calls into the library for one batch: per-sample %d, batched %d.\n\n" % (sum(counts["per_sample"].values()), sum(counts["batched"].values())))
            f.write("| entry point | per-sample | batched |\n|---|---|---|\n")
            for n in names:
                f.write("| `%s` | %d | %d |\n" % (n, counts["per_sample"][n], counts["batched"][n]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
