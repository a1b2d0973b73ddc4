"""conv_wino's tile edges: the columns beside a tile (x0 - 1 and x0 + TW) reach the input transform of the tile's first and last quad.
In the persistent kernel they are loaded and activated by the staging waves' EDGE lanes (one per (patch row, channel group) row and
side, behind the main lanes of each wave) and fetched with ds_bpermute; the one-tile kernel keeps a fifth value per lane.  Both forms run
here (route levels 8 and 2) on shapes whose tiles have every kind of edge:

    B  C   H x W    Cout
    1  16   8 x 32  128   one tile column: both edges are the image border (zero, with zero coefficients under a deferred norm)
    2  20   8 x 64  128   interior edges on both sides; 12 zero-weight channels behind the 20 real ones in the second chunk
    1  32  16 x 16  128   the 16-column geometry (10 patch rows x 4 quads per staging wave, 20 edge lanes)
    1  16   8 x 32  256   two output-channel blocks: two items stream through one workgroup

Every launch reads from a NaN-fenced buffer in which every OTHER sample is NaN as well, sample by sample: a load at a wrong edge offset,
or one that leaves the sample's range (the zero-weight channel tail reads past it and must be clamped to zero), poisons the output.

References and bars.  Plain form: the split-exact fp64 reference of tests/_split_exact.py (wino_split_reference) at the project's
SPLIT_BAR 2^-18 A, and the fp64 convolution of the true operands at 2e-5 max(max|y|, 1), the bars of test_gpu_wino_stream_routes.py and
test_gpu_wino.py for the plain forms.  Deferred normalisation (GroupNorm(4) + GELU, in_slope < 0; InstanceNorm + LeakyReLU 0.01): the
kernel normalises in fp32, so the split-exact reference does not apply -- fp64 of the materialised activation at 3e-5 and the two-pass route
(group_norm_apply, then the same kernel form) at 2e-5, the PRE bars of those two modules.  A wrong or missing edge column is an O(0.1)
error per output of the tile's first or last column pair at these shapes, four orders above either bar."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from _split_exact import SPLIT_BAR, TORCH_ACT, randn, ratio, wino_split_reference

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 8, 32, 128), (2, 20, 8, 64, 128), (1, 32, 16, 16, 128), (1, 16, 8, 32, 256)]
LEVELS = (8, 2)
FENCE = 4          # floats: keeps the view 16-byte aligned


@contextlib.contextmanager
def wino_forced(level):
    from cineflow._lib import lib
    prev = lib().cf_conv_wino_enable(level)
    try:
        yield
    finally:
        lib().cf_conv_wino_enable(prev)


def alone(x, b, dev):
    """x on the device inside a NaN fence with every sample but b set to NaN"""
    buf = torch.full((x.numel() + 2 * FENCE,), float("nan"), device=dev)
    xd = buf[FENCE:FENCE + x.numel()].view(x.shape)
    xd[b] = x[b].to(dev)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 0
    return xd


_OPS = {}


def operands(B, C, H, W, Cout):
    key = (B, C, H, W, Cout)
    if key not in _OPS:
        k = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
        x = randn(B, C, H, W, seed=700 + C + W) * (1.0 + 0.2 * k) + 0.1 * k - 0.3
        g, bt = 1 + 0.3 * randn(C, seed=701), 0.3 * randn(C, seed=702)
        w = randn(Cout, C, 3, 3, seed=703) / math.sqrt(C * 9)
        b = randn(Cout, seed=704)
        _OPS[key] = (x, g, bt, w, b)
    return _OPS[key]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("B,C,H,W,Cout", SHAPES)
def test_wino_plain_edges(dev, B, C, H, W, Cout, level):
    from cineflow import ops
    x, _, _, w, b = operands(B, C, H, W, Cout)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    ref = wino_split_reference(x, w, b, s)
    bar = SPLIT_BAR * ref["A"]
    scale = max(float(ref["true"].abs().max()), 1.0)
    with wino_forced(level):
        assert ops.wino_form(B, C, 0, H, W, Cout) == level, "route level %d no longer takes this shape" % level
        for smp in range(B):
            out = ops.conv2d_wino(alone(x, smp, dev), wpk, s, b.to(dev), Cout)
            o = out[smp].cpu().double()
            assert bool(torch.isfinite(o).all()), "a load left the sample's range"
            worst, d = ratio(o, ref["y3"][smp], bar[smp]), float((o - ref["true"][smp]).abs().max())
            print("\nconv_wino edges %dx%dx%dx%d -> %d level %d sample %d: |out - y3| / (2^-18 A) = %.4f, max|out - fp64| = %.2e (bar %.1e)"
                  % (B, C, H, W, Cout, level, smp, worst, d, 2e-5 * scale), end="")
            assert worst <= 1.0, ("split-exact", worst)
            assert d <= 2e-5 * scale, ("fp64 contract", d)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("act", ["gelu", "lrelu"])
@pytest.mark.parametrize("B,C,H,W,Cout", SHAPES)
def test_wino_prenorm_edges(dev, B, C, H, W, Cout, act, level):
    from cineflow import ops
    x, g, bt, w, b = operands(B, C, H, W, Cout)
    groups, slope = (4, -1.0) if act == "gelu" else (C, 0.01)
    xs = x.double().view(B, groups, -1)
    ws = torch.stack([xs.sum(-1), (xs ** 2).sum(-1)], -1).reshape(-1).to(dev)
    gd, btd, bd = g.to(dev), bt.to(dev), b.to(dev)
    coef = ops.group_norm_coef(ws, gd, btd, groups, B, C, H * W)
    want = F.conv2d(TORCH_ACT[act](F.group_norm(x.double(), groups, g.double(), bt.double(), eps=1e-5)), w.double(), b.double(), padding=1)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    with wino_forced(level):
        assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=True) == level, "route level %d no longer takes this shape" % level
        two = ops.conv2d_wino(ops.group_norm_apply(x.to(dev), gd, btd, groups, ws, act=act, out=torch.empty(x.shape, device=dev)), wpk, s, bd, Cout)
        for smp in range(B):
            out = ops.conv2d_wino_prenorm(alone(x, smp, dev), coef, slope, wpk, s, bd, Cout)
            o = out[smp]
            assert bool(torch.isfinite(o).all()), "a load left the sample's range"
            d, d2 = float((o.cpu().double() - want[smp]).abs().max()), float((o - two[smp]).abs().max())
            print("\nconv_wino PRE edges %dx%dx%dx%d -> %d %s level %d sample %d: max|out - fp64| = %.2e (bar 3e-5), max|out - two-pass| = %.2e (bar 2e-5)"
                  % (B, C, H, W, Cout, act, level, smp, d, d2), end="")
            assert d <= 3e-5, (act, d)
            assert d2 <= 2e-5, (act, d2)
