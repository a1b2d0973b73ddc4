"""Scoring every two-model ensemble of one validation case: one cf_ensemble_pairs launch against the chained route.

Workload: one synthetic case of the edt_bench volume (160 x 384 x 384, the crop is the volume), K = 4, fp16, M = 4 members -> 6 pairs.
Members are seeded softmaxes of blocky logits (tools/ensemble_bench.py's: large confident regions with noisy borders), the ground truth is
the arg-max of a fifth such softmax, so the confusion is concentrated in a few bins as a real one is.

    (a) pairs    one ops.ensemble_pairs call: 6 label volumes and 6 label confusions
    (b) chained  the route without the kernel, for the same result: six ops.ensemble_merge calls and six cf_label_confusion calls

Both work on device-resident members into preallocated outputs and are timed by device events around `--calls` back-to-back calls; the two
routes alternate, one sample each per round, `--runs` rounds after a warm-up round, medians reported with every sample.  Bytes are what a
route must move: (a) M x K x voxels x 2 read + voxels (ground truth) + 6 x voxels written; (b) 6 x (2 x K x voxels x 2 read + voxels
written) + 6 x 2 x voxels read.  Results are compared before timing.

    python tools/model_selection_bench.py [--calls 5] [--runs 5] [--small]      one JSON line, then the clocks rocm-smi reports"""
import argparse
import json
import os
import statistics
import sys
from itertools import combinations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K, M = 4, 4
VOLUME = (160, 384, 384)
SMALL = (6, 48, 40)                       # --small: a rehearsal of the script, not a measurement
HIST_K = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "model_selection_bench needs a GPU"
    from cineflow import ops
    from cineflow._lib import check, lib
    from ensemble_bench import blocky_softmax, smi
    dev = torch.device("cuda:0")
    full = SMALL if a.small else VOLUME
    voxels = full[0] * full[1] * full[2]
    print(json.dumps({"clocks_before": smi()}), flush=True)
    members = [torch.from_numpy(blocky_softmax(K, full, 60 + i)).to(dev) for i in range(M)]
    gt = torch.from_numpy(blocky_softmax(K, full, 59).argmax(0).astype(np.uint8)).to(dev)
    pairs = list(combinations(range(M), 2))
    P = len(pairs)
    seg_a = torch.empty((P,) + full, dtype=torch.uint8, device=dev)
    hist_a = torch.empty((P, HIST_K * HIST_K + 1), dtype=torch.int64, device=dev)
    seg_b = torch.empty((P,) + full, dtype=torch.uint8, device=dev)
    hist_b = torch.empty((P, HIST_K * HIST_K + 1), dtype=torch.int64, device=dev)

    def route_a():
        ops.ensemble_pairs(members, pairs, gt, out=(seg_a, hist_a))

    def route_b():
        for p, (i, j) in enumerate(pairs):
            ops._ensemble_merge_into([members[i], members[j]], seg_b[p], (0, 0, 0), None, None)
            check(lib().cf_label_confusion(seg_b[p].data_ptr(), gt.data_ptr(), voxels, HIST_K, hist_b[p].data_ptr(), None), "cf_label_confusion")

    route_a()
    route_b()
    torch.cuda.synchronize()
    equal = bool(torch.equal(seg_a, seg_b)) and bool(torch.equal(hist_a, hist_b))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(route):
        e0.record()
        for _ in range(a.calls):
            route()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.calls

    ta, tb = [], []
    for r in range(a.runs + 1):                                                   # the first round is the warm-up
        first, second = (route_a, route_b) if r % 2 == 0 else (route_b, route_a)   # alternate, and alternate who goes first
        x, y = sample(first), sample(second)
        if r:
            ta.append(x if first is route_a else y)
            tb.append(y if first is route_a else x)
    ma, mb = statistics.median(ta), statistics.median(tb)
    bytes_a = M * K * voxels * 2 + voxels + P * voxels
    bytes_b = P * (2 * K * voxels * 2 + voxels) + P * 2 * voxels
    print(json.dumps({"volume": full, "K": K, "M": M, "pairs": P, "calls_per_sample": a.calls, "results_equal": equal,
                      "pairs_ms": round(ma * 1e3, 3), "pairs_samples_ms": [round(t * 1e3, 3) for t in ta],
                      "chained_ms": round(mb * 1e3, 3), "chained_samples_ms": [round(t * 1e3, 3) for t in tb],
                      "chained_spread_ms": round((max(tb) - min(tb)) * 1e3, 3), "chained_over_pairs": round(mb / ma, 3),
                      "pairs_bytes": bytes_a, "pairs_GBs": round(bytes_a / ma / 1e9, 1),
                      "chained_bytes": bytes_b, "chained_GBs": round(bytes_b / mb / 1e9, 1),
                      "pairs_not_slower_than_chained_plus_spread": bool(ma <= mb + (max(tb) - min(tb)))}), flush=True)
    print(json.dumps({"clocks_after": smi()}), flush=True)


if __name__ == "__main__":
    main()
