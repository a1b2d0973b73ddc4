"""conv3d_pw_f16s_kernel (csrc/conv3d_pw_f16s.hip), the strided (1,1,1) convolution of a residual block's skip projection, against a
split-exact fp64 reference, one row per thing the kernel can get wrong.

Reference and bars are those of test_gpu_conv3d_routes.py with F.conv3d(stride, no padding) on the exact operands the kernel multiplies:
    y3 = 2^-s (conv3d(xh, wl) + conv3d(xl, wh) + conv3d(xh, wh)) + b          in float64
    |out - y3| <= 2^-18 A,   A = 2^-s conv3d(|xh| + |xl|, |wh| + |wl|) + |b|
The accumulator sees one MFMA per 16-channel k-step and term: at most 20 per term, 60 with the lo terms (Cin = 320), inside the n <= 63
range for which the 2-D derivation gives (n + 1) u A <= 64 u A with certainty.  What the bar resolves is asserted per row: the one-term
reference y1 fails it and a reference without the last input channel fails it.  Next to it the suite's standing 1e-5 against the fp64
convolution of the true operands, the gn_ws statistics with groups = Cout at 2e-6, sentinel floats around the output, and the probe must
say 1 for the row -- otherwise nothing would have been tested.  Rows with bias=False pass a null bias, as the reference layer does
(conv_blocks.py:127).  The worst ratio to the bar is printed per row (pytest -s).
"""
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from _split_exact import SPLIT_BAR, check_stats, device_input, randn, ratio
from _split_exact import split_reference_3d as split_reference

pytestmark = pytest.mark.gpu

Row = namedtuple("Row", "n B Cin D H W Cout stride bias view")
ROWS = [
    Row(1, 2, 40, 5, 13, 11, 72, (2, 2, 2), True, False),      # odd sizes; channel tails 40 = 2 * 16 + 8 and 72 = 2 * 32 + 8
    Row(2, 2, 40, 4, 12, 20, 48, (2, 2, 2), True, False),      # even sizes: the last plane, row and column are never read
    Row(3, 2, 40, 3, 13, 11, 72, (1, 2, 2), True, False),      # in-plane stride only
    Row(4, 2, 72, 4, 7, 6, 72, (2, 1, 1), True, False),        # depth stride only
    Row(5, 2, 40, 3, 6, 10, 72, (1, 1, 1), True, False),       # no stride
    Row(6, 1, 4, 8, 32, 32, 8, (1, 2, 2), False, False),       # fixture shape (ref_model_folder_resenc, stage 1), null bias
    Row(7, 1, 8, 8, 16, 16, 16, (2, 2, 2), False, False),      # fixture shape (stage 2), null bias
    Row(8, 3, 320, 2, 4, 5, 320, (2, 2, 2), True, False),      # six outputs per sample: several samples per workgroup, statistics across samples;
                                                               # 20 k-steps, 60 MFMAs with the lo terms
    Row(9, 2, 256, 4, 8, 8, 320, (2, 2, 2), True, False),      # Cout 320 = 2 * 128 + 64
    Row(10, 2, 40, 5, 13, 11, 72, (2, 2, 2), True, True),      # row 1, input one float into a NaN-fenced buffer
    Row(11, 23, 40, 2, 4, 5, 72, (2, 2, 2), True, False),      # six outputs per sample, 21 samples per workgroup: a second workgroup whose
                                                               # group of samples the batch cuts short (2 of 21)
]


def row_id(r):
    return "row%d_s%d%d%s" % (r.n, r.stride[0], r.stride[1], "_view" if r.view else "")


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_conv3d_pw_f16s_route(dev, row):
    from cineflow import ops
    B, Cin, D, H, W, Cout, st = row.B, row.Cin, row.D, row.H, row.W, row.Cout, row.stride
    seed = 2000 * (1 if row.view else row.n) + 10 * st[0] + st[1]          # the view row multiplies row 1's operands
    x = randn(B, Cin, D, H, W, seed=seed)
    w = randn(Cout, Cin, 1, 1, 1, seed=seed + 1) / math.sqrt(Cin)
    b = randn(Cout, seed=seed + 2) if row.bias else torch.zeros(Cout)
    assert ops.conv3d_pw_f16s_ok(B, Cin, D, H, W, Cout, st), "the probe declines the row: nothing would be tested"
    xd = device_input(x, dev, row.view)
    wpk, s = ops.pack_conv3d_pw_weight_f16s(w.to(dev))
    ref = split_reference(x, w, b, s, lambda a, m: F.conv3d(a, m, stride=st))
    shape = tuple(ref["y3"].shape)
    assert shape == (B, Cout, (D - 1) // st[0] + 1, (H - 1) // st[1] + 1, (W - 1) // st[2] + 1)
    n, fence = ref["y3"].numel(), 64
    buf = torch.full((n + 2 * fence,), 7.0, device=dev)
    out, ws = ops.conv3d_pw_f16s(xd, wpk, s, b.to(dev) if row.bias else None, Cout, st, out=buf[fence:fence + n].view(shape), stats_groups=Cout)
    torch.cuda.synchronize()
    assert bool((buf[:fence] == 7.0).all()) and bool((buf[fence + n:] == 7.0).all()), "floats around the output were written"
    o = out.cpu().double()
    bar = SPLIT_BAR * ref["A"]
    worst = ratio(o, ref["y3"], bar)
    print("\n%s worst |out - y3| / (2^-18 A) = %.4f" % (row_id(row), worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0, "the bar does not resolve the lo terms"
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    d = float((o - ref["true"]).abs().max())
    assert d <= 1e-5, ("fp64 contract", d)
    check_stats(out.cpu(), ws, B, Cout, list(range(B)))


def test_probe_declines_one_term_mode(dev):
    """only the three-term product is built: under cf_conv_terms(1) the caller keeps its composition"""
    from cineflow import ops
    assert ops.conv3d_pw_f16s_ok(2, 40, 5, 13, 11, 72, (2, 2, 2))
    with ops.conv_terms(1):
        assert not ops.conv3d_pw_f16s_ok(2, 40, 5, 13, 11, 72, (2, 2, 2))
    assert ops.conv3d_pw_f16s_ok(2, 40, 5, 13, 11, 72, (2, 2, 2))
    assert not ops.conv3d_pw_f16s_ok(2, 40, 5, 13, 11, 72, (3, 2, 2))
