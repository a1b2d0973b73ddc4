"""conv3d_f16s_kernel (csrc/conv3d_f16s.hip) against a split-exact fp64 reference, one row per thing the kernel can get wrong.

Reference.  As in test_gpu_conv_f16s_routes.py, with F.conv3d on the exact operands the kernel multiplies:
    s, wh, wl        as pack_conv3d_weight_f16s makes them: ws = 2^s w (exact), wh = fp16(ws), wl = fp16(ws - wh)
    xh, xl           xh = fp16(x), xl = fp16(x - xh)
    y3 = 2^-s (conv3d(xh, wl) + conv3d(xl, wh) + conv3d(xh, wh)) + b
evaluated in float64.  Products of fp16 values are exact in fp32 and the 2^-s scaling is exact, so the kernel differs from y3 only by the
rounding of its fp32 accumulation.

Bar.  |out - y3| <= 2^-18 A with A = 2^-s conv3d(|xh| + |xl|, |wh| + |wl|) + |b|.  The accumulator sees n = chunks x kd x 9 MFMAs per term;
the largest rows here have 3 chunks x 27 taps = 81 per term, 243 with the lo terms.  That is past the n <= 63 for which the 2-D derivation
gives 64 u A with certainty ((n + 1) u A, u = 2^-24), and well inside the random-walk range (sqrt(n) u A, n up to ~4000) which the 2-D
tables already rely on.  What the bar resolves is asserted per row: the one-term reference y1 fails it (the lo terms are there), a
reference without the last input channel fails it, and on the kd = 3 rows a reference without the depth tap dz = 0 fails it.  (Row 10
has D = 1: the dz = 0 tap reads the plane -1 of every output plane, its split-exact contribution is exactly zero and no bar can see it;
that row asserts the zero instead.)  The worst ratio to the bar is printed per row (pytest -s).

Next to it: the suite's standing 1e-5 absolute bound against the fp64 convolution of the true operands; the gn_ws statistics with
groups = Cout against fp64 sums of the stored output at the suite's 2e-6; the output lives inside a larger sentinel-filled buffer whose
floats before and after it must stay untouched; and ops.conv3d_f16s_ok must say 1 for the row -- otherwise a fallback would be passing.
"""
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from _split_exact import SPLIT_BAR, check_stats, device_input, randn, ratio
from _split_exact import split_reference_3d as split_reference

pytestmark = pytest.mark.gpu

Row = namedtuple("Row", "n B C1 C2 D H W Cout k stride view")
ROWS = [
    Row(1, 2, 40, 0, 5, 12, 20, 48, (3, 3, 3), (1, 1, 1), False),    # interior planes + both depth borders; channel tail 40 = 2 * 16 + 8
    Row(2, 2, 40, 0, 3, 12, 20, 48, (1, 3, 3), (1, 1, 1), False),    # no depth taps
    Row(3, 2, 40, 0, 5, 13, 11, 72, (3, 3, 3), (2, 2, 2), False),    # odd sizes, Do = 3; Cout tail 72 = 2 * 32 + 8
    Row(4, 2, 40, 0, 4, 12, 20, 48, (3, 3, 3), (2, 2, 2), False),    # even D: the last output plane loses its far tap
    Row(5, 2, 40, 0, 4, 12, 20, 48, (3, 3, 3), (1, 2, 2), False),    # anisotropic pooling convolution
    Row(6, 1, 40, 0, 3, 13, 11, 48, (1, 3, 3), (1, 2, 2), False),    # the same, odd in-plane
    Row(7, 2, 24, 16, 4, 8, 12, 40, (3, 3, 3), (1, 1, 1), False),    # two inputs, C1 not a chunk multiple (split-aware packing)
    Row(8, 2, 1, 0, 4, 16, 20, 32, (1, 3, 3), (1, 1, 1), False),     # first layer, one modality
    Row(8, 2, 1, 0, 4, 16, 20, 32, (3, 3, 3), (1, 1, 1), False),
    Row(9, 3, 40, 0, 2, 4, 5, 320, (3, 3, 3), (1, 1, 1), False),     # bottleneck: several planes / samples per workgroup, 320 = 2 * 128 + 64,
                                                                    # two valid depth taps per plane; statistics when a workgroup spans samples
    Row(10, 2, 40, 0, 1, 6, 12, 48, (3, 3, 3), (1, 1, 1), False),    # D = 1: centre tap only
    Row(11, 2, 40, 0, 5, 12, 20, 48, (3, 3, 3), (1, 1, 1), True),    # row 1, input one float into a NaN-fenced buffer
    Row(12, 2, 40, 0, 5, 12, 20, 48, (3, 3, 3), (2, 1, 1), False),   # depth stride 2 at in-plane stride 1 (BasicResidualBlock3D), odd D
    Row(13, 2, 40, 0, 4, 12, 20, 48, (3, 3, 3), (2, 1, 1), False),   # the same, even D: the last output plane loses its far tap
]


def row_id(r):
    return "row%d_k%d_s%d%d%s" % (r.n, r.k[0], r.stride[0], r.stride[1], "_view" if r.view else "")


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_conv3d_f16s_route(dev, row):
    from cineflow import ops
    B, C1, C2, D, H, W, Cout, k, st = row.B, row.C1, row.C2, row.D, row.H, row.W, row.Cout, row.k, row.stride
    C = C1 + C2
    seed = 1000 * row.n + 10 * k[0] + st[0]
    x = randn(B, C, D, H, W, seed=seed)
    w = randn(Cout, C, *k, seed=seed + 1) / math.sqrt(C * k[0] * 9)
    b = randn(Cout, seed=seed + 2)
    assert ops.conv3d_f16s_ok(B, C1, C2, D, H, W, Cout, k, st), "the probe declines the row: the fallback would be passing this test"
    x1d = device_input(x[:, :C1].contiguous(), dev, row.view)
    x2d = x[:, C1:].contiguous().to(dev) if C2 else None
    wpk, s = ops.pack_conv3d_weight_f16s(w.to(dev), c1=C1 if C2 else None)
    pad = (k[0] // 2, 1, 1)
    ref = split_reference(x, w, b, s, lambda a, m: F.conv3d(a, m, stride=st, padding=pad))
    shape = tuple(ref["y3"].shape)
    n, fence = ref["y3"].numel(), 64
    buf = torch.full((n + 2 * fence,), 7.0, device=dev)
    out, ws = ops.conv3d_f16s(x1d, wpk, s, b.to(dev), Cout, k, st, x2=x2d, out=buf[fence:fence + n].view(shape), stats_groups=Cout)
    torch.cuda.synchronize()
    assert bool((buf[:fence] == 7.0).all()) and bool((buf[fence + n:] == 7.0).all()), "floats around the output were written"
    o = out.cpu().double()
    bar = SPLIT_BAR * ref["A"]
    worst = ratio(o, ref["y3"], bar)
    print("\n%s worst |out - y3| / (2^-18 A) = %.4f" % (row_id(row), worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0, "the bar does not resolve the lo terms"
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    if k[0] == 3:
        if D > 1:
            assert ratio(o, ref["y3"] - ref["z3"], bar) > 1.0, "a dropped depth tap dz = 0 would pass the bar"
        else:
            assert float(ref["z3"].abs().max()) == 0.0
    d = float((o - ref["true"]).abs().max())
    assert d <= 1e-5, ("fp64 contract", d)
    check_stats(out.cpu(), ws, B, Cout, list(range(B)))
