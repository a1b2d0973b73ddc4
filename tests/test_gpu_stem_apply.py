"""The stem DoubleConv without its stored shortcut map: cf_stem_block_y (the stem launch with the stores of r compiled out) and
cf_group_norm_apply_res_stem (the block's final pass, which rebuilds r = conv1x1(x) per element).

Nothing here has a tolerance of its own except the fp64 sums: y and the applied output are held BITWISE to the stored-r path
(cf_stem_block, cf_group_norm_apply_res_norm on the r it stored, the same workspaces), which test_gpu_stem_block.py and
test_gpu_ops.py hold to fp64 references.  The statistics of two launches differ by the order of their fp64 atomics alone (a block's
contribution is formed in a fixed order): 1e-12 relative.  A bitwise mismatch of the output means the FMA order of the rebuilt r, or
the expression behind it, differs from the stored path's.

Shapes: non-square with H * W >= 2048 (three 1024-pixel segments per sample); an odd batch; H * W < 2048, which the apply's probe
declines (a workgroup walks all channels of 1024 pixels: below two segments per sample the grid is too small to be worth it), so the
block keeps the stored-r path there.  Cin 1 and 6, 64 channels, 8 groups, GELU, both residual modes.  The block row holds one forward
of the stem route against the oracle's DoubleConv at test_gpu_deferred_norm_blocks.py's bar (2e-5) and asserts through the recorded
ops calls that no r was allocated."""
import math

import pytest
import torch

import test_gpu_deferred_norm_blocks as DN
from _split_exact import randn

pytestmark = pytest.mark.gpu

GROUPS = 8
COUT = 64
SHAPES = [(2, 48, 64), (3, 64, 64), (2, 16, 48)]
CASES = [(cin, B, H, W) for cin in (1, 6) for (B, H, W) in SHAPES]
FENCE = 64


def params(cin):
    w3 = randn(COUT, cin, 3, 3, seed=401) / math.sqrt(9 * cin)
    w1 = randn(COUT, cin, 1, 1, seed=402) / math.sqrt(cin)
    b3, b1 = randn(COUT, seed=403), randn(COUT, seed=404)
    g2, be2, gr, ber = (1.0 + 0.1 * randn(COUT, seed=405), 0.1 * randn(COUT, seed=406), 1.0 + 0.1 * randn(COUT, seed=407), 0.1 * randn(COUT, seed=408))
    return w3, b3, w1, b1, g2, be2, gr, ber


def stats_of(t, B):
    """fp64 {sum, sum of squares} per (sample, group) of a device map, as a statistics workspace holds them"""
    v = t.double().view(B, GROUPS, -1)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1).reshape(-1).contiguous()


def fenced(shape, dev):
    """a NaN-filled buffer with sentinel fences on both sides of the view that the kernel is given"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * FENCE,), 12345.0, device=dev)
    view = buf[FENCE:FENCE + n].view(shape)
    view.fill_(float("nan"))
    return buf, view


@pytest.mark.parametrize("cin,B,H,W", CASES)
def test_stem_block_y_equals_stem_block(dev, cin, B, H, W):
    from cineflow import ops
    x = DN.sample_input(B, cin, H, W, 410 + cin).to(dev)
    w3, b3, w1, b1 = (t.to(dev) for t in params(cin)[:4])
    y, ws_y, r, ws_r = ops.stem_block(x, w3, b3, w1, b1, GROUPS)
    yy, ws_yy, ws_ry = ops.stem_block_y(x, w3, b3, w1, b1, GROUPS)
    torch.cuda.synchronize()
    assert torch.equal(y, yy)
    for what, a, b in (("ws_y", ws_y, ws_yy), ("ws_r", ws_r, ws_ry)):
        rel = float(((a - b).abs() / a.abs()).max())
        print("\nstem_block_y Cin %d B %d %dx%d: %s differs by %.2e relative (bar 1e-12)" % (cin, B, H, W, what, rel))
        assert rel <= 1e-12, (what, rel)
    # and ws_r is the statistics of the map that was not stored
    want = stats_of(r, B)
    assert float(((ws_ry - want).abs() / (r.double().abs().view(B, GROUPS, -1).sum(-1).repeat_interleave(2) + 1.0)).max()) <= 2e-6
    # no bias
    y0, _, r0, ws_r0 = ops.stem_block(x, w3, None, w1, None, GROUPS)
    yy0, _, ws_ry0 = ops.stem_block_y(x, w3, None, w1, None, GROUPS)
    assert torch.equal(y0, yy0) and float(((ws_r0 - ws_ry0).abs() / ws_r0.abs().clamp_min(1e-300)).max()) <= 1e-12


@pytest.mark.parametrize("mode", ["after_act", "before_act"])
@pytest.mark.parametrize("cin,B,H,W", CASES)
def test_apply_res_stem_is_the_stored_path_bit_for_bit(dev, cin, B, H, W, mode):
    from cineflow import ops
    x = DN.sample_input(B, cin, H, W, 410 + cin).to(dev)
    w3, b3, w1, b1, g2, be2, gr, ber = (t.to(dev) for t in params(cin))
    _, _, r, ws_r = ops.stem_block(x, w3, b3, w1, b1, GROUPS)
    y2 = (DN.sample_input(B, COUT, H, W, 420 + cin) * 1.5 + 0.3).to(dev)          # conv2's raw map: any map with its statistics
    ws2 = stats_of(y2, B)
    if H * W < 2048:
        assert not ops.group_norm_apply_res_stem_ok(x, COUT, GROUPS)
        with pytest.raises(RuntimeError):
            ops.group_norm_apply_res_stem(y2, g2, be2, GROUPS, ws2, x, w1, b1, ws_r, gr, ber, act="gelu", res_mode=mode, out=torch.empty_like(y2))
        return
    assert ops.group_norm_apply_res_stem_ok(x, COUT, GROUPS)
    want = ops.group_norm_apply(y2, g2, be2, GROUPS, ws2, act="gelu", res=r, res_mode=mode, res_norm=(ws_r, gr, ber), out=torch.empty_like(y2))
    buf, out = fenced(tuple(y2.shape), dev)
    got = ops.group_norm_apply_res_stem(y2, g2, be2, GROUPS, ws2, x, w1, b1, ws_r, gr, ber, act="gelu", res_mode=mode, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:FENCE] == 12345.0).all()) and bool((buf[-FENCE:] == 12345.0).all()), "the kernel wrote outside its output"
    assert not bool(torch.isnan(out).any()), "the kernel left part of its output unwritten"
    assert torch.equal(out, want), "max difference %.3e: the rebuilt r or the expression behind it is not the stored path's" % float((out - want).abs().max())
    # no bias on the 1x1 shortcut, no affine parameters, in place
    _, _, r0, ws_r0 = ops.stem_block(x, w3, b3, w1, None, GROUPS)
    want0 = ops.group_norm_apply(y2, None, None, GROUPS, ws2, act="gelu", res=r0, res_mode=mode, res_norm=(ws_r0, None, None), out=torch.empty_like(y2))
    inplace = y2.clone()
    got0 = ops.group_norm_apply_res_stem(inplace, None, None, GROUPS, ws2, x, w1, None, ws_r0, None, None, act="gelu", res_mode=mode, out=inplace)
    assert torch.equal(got0, want0)


@pytest.fixture
def stem_calls(monkeypatch):
    """the recorded calls of the ops that allocate or consume a shortcut map, in order"""
    from cineflow import ops
    log = []

    def counting(name, real):
        def f(*a, **k):
            log.append(name)
            return real(*a, **k)
        return f
    for name in ("stem_block", "stem_block_y", "group_norm_apply", "group_norm_apply_res_stem", "conv2d_small_cin"):
        monkeypatch.setattr(ops, name, counting(name, getattr(ops, name)))
    return log


@pytest.mark.parametrize("cin,B,H,W", CASES)
def test_double_conv_stem_route_against_the_oracle(dev, stem_calls, cin, B, H, W):
    from cineflow.nn import DoubleConv
    from oracle import models as OM
    m, ora = DN.filled(DoubleConv(cin, COUT, True, 1), OM.DoubleConv(cin, COUT, True, 1), 430 + cin, dev)
    x = DN.sample_input(B, cin, H, W, 431 + cin)
    ref = DN.reference(("stem_apply", cin, B, H, W), ora, x)
    with DN.conv_mode("f16s"):
        out = DN.run_unchanged(m, x.to(dev))
    DN.check("DoubleConv stem Cin %d B %d %dx%d" % (cin, B, H, W), out, ref, DN.BLOCK_BAR)
    if H * W < 2048:          # declined: the stored-r path, as before
        assert stem_calls.count("stem_block") == 1 and "stem_block_y" not in stem_calls and "group_norm_apply_res_stem" not in stem_calls
        return
    # no r anywhere: neither stem_block nor a 1x1 convolution ran, and the final pass is the rebuilding one
    assert stem_calls.count("stem_block_y") == 1 and stem_calls.count("group_norm_apply_res_stem") == 1, stem_calls
    assert "stem_block" not in stem_calls and "conv2d_small_cin" not in stem_calls and stem_calls[-1] == "group_norm_apply_res_stem", stem_calls
