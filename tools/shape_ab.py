#!/usr/bin/env python3
"""A/B of conv_f16s routing switches on a few layer shapes: run once per environment setting (the switches are read once per process).
  CF_CONV_STREAM=0 python tools/shape_ab.py        # prints one line per case: plain conv (+ fused statistics) and the prenorm variant
Cases: (B, C1, C2, H, Cout, act) -- the U-Net's 32 / 64-channel layers at B = 240 frames, the flow net's 64-channel layers at B = 128."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from cineflow import ops  # noqa: E402
from microbench import timeit  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
knobs = " ".join("%s=%s" % (k, v) for k, v in sorted(os.environ.items()) if k.startswith("CF_"))
print("== knobs: %s" % (knobs or "(default)"))
CASES = [(240, 32, 0, 256, 32, "lrelu"), (240, 32, 32, 256, 32, None), (240, 64, 0, 128, 64, "lrelu"), (128, 64, 0, 256, 64, "gelu"), (128, 64, 64, 256, 64, None),
         (128, 81, 0, 256, 64, None), (480, 480, 0, 16, 480, "lrelu"), (480, 480, 480, 16, 480, None), (128, 128, 0, 128, 128, "gelu")]
if len(sys.argv) > 1:
    CASES = [c for i, c in enumerate(CASES) if str(i) in sys.argv[1:]]
for (B, C1, C2, H, Cout, act) in CASES:
    x1 = torch.randn(B, C1, H, H, generator=g).to(dev)
    x2 = torch.randn(B, C2, H, H, generator=g).to(dev) if C2 else None
    w = (torch.randn(Cout, C1 + C2, 3, 3, generator=g) / math.sqrt((C1 + C2) * 9)).to(dev)
    wpk, wsc = ops.pack_conv_weight_f16s(w, c1=C1 if (C2 and C1 % 16) else None)
    groups = Cout if act == "lrelu" else 8
    flops = 2.0 * B * H * H * Cout * (C1 + C2) * 9
    t = timeit(lambda: ops.conv2d_f16s(x1, wpk, wsc, None, Cout, 3, 3, 1, (1, 1), x2=x2, stats_groups=groups))
    line = "  B%3d C%3d+%-3d %3dx%-3d -> %3d | conv+stats %8.1f us %6.1f TF" % (B, C1, C2, H, H, Cout, t * 1e6, flops / t / 1e12)
    if act and not C2 and ops.prenorm_ok(x1, Cout):
        _, ws = ops.conv2d_f16s(x1, wpk, wsc, None, Cout, 3, 3, 1, (1, 1), stats_groups=groups)
        coef = ops.group_norm_coef(ws.clone(), None, None, groups, B, C1, H * H)
        tp = timeit(lambda: ops.conv2d_f16s_prenorm(x1, coef, 0.01 if act == "lrelu" else -1.0, wpk, wsc, None, Cout, stats_groups=groups))
        line += " | prenorm(%s) %8.1f us %6.1f TF" % (act, tp * 1e6, flops / tp / 1e12)
    print(line, flush=True)
    del x1, x2
    torch.cuda.empty_cache()
