"""cf_stem_block: conv1 (3x3 pad 1) and the 1x1 downsample convolution of a stem DoubleConv in one launch, with the GroupNorm statistics of both.

Reference: torch.nn.functional.conv2d in fp64 on the CPU, at the bar tests/test_gpu_ops.py holds conv2d_small_cin to (5e-6: exact fp32 FMA
chains of <= 54 O(1) products); statistics against fp64 sums of the kernel's OWN outputs at that test's 2e-6 of the group's absolute sum.
The kernel has no grid loop -- a workgroup owns one 64 x (4 PY) tile of one sample and the grid covers the map -- so the wide case takes
several column tiles (and, at 6 channels, row tiles) per sample instead of a second trip of one workgroup."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GROUPS = 8
COUT = 64
MAPS = [(8, 12), (20, 36), (33, 20)]          # smaller than one tile; tiles that end inside the image; odd height (and width % 4 != 0 rows of stores)
CASES = [(cin, B, H, W) for cin in (1, 6) for B in (2, 3) for (H, W) in MAPS] + [(1, 2, 40, 200), (6, 2, 40, 200)]   # wide: four column tiles


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


_IN = {}


def inputs(cin, B, H, W):
    """(x, w3, b3, w1, b1, fp64 3x3 reference, fp64 1x1 reference), computed once per case"""
    key = (cin, B, H, W)
    if key not in _IN:
        x = randn(B, cin, H, W, seed=300 + cin)
        w3 = randn(COUT, cin, 3, 3, seed=301) / math.sqrt(9 * cin)
        w1 = randn(COUT, cin, 1, 1, seed=302) / math.sqrt(cin)
        b3, b1 = randn(COUT, seed=303), randn(COUT, seed=304)
        y = F.conv2d(x.double(), w3.double(), b3.double(), padding=1)
        r = F.conv2d(x.double(), w1.double(), b1.double())
        _IN[key] = (x, w3, b3, w1, b1, y, r)
    return _IN[key]


def stats_error(ws, out, B):
    yo = out.cpu().double()
    want = torch.stack([yo.view(B, GROUPS, -1).sum(-1), (yo ** 2).view(B, GROUPS, -1).sum(-1)], -1)
    scale = yo.abs().view(B, GROUPS, -1).sum(-1)[..., None] + 1.0
    return float(((ws.cpu().view(B, GROUPS, 2) - want).abs() / scale).max())


@pytest.mark.parametrize("cin,B,H,W", CASES)
def test_stem_block(dev, cin, B, H, W):
    from cineflow import ops
    x, w3, b3, w1, b1, y_ref, r_ref = inputs(cin, B, H, W)
    xd, w3d, b3d, w1d, b1d = (t.to(dev) for t in (x, w3, b3, w1, b1))
    assert ops.stem_block_ok(xd, COUT, GROUPS)
    y, ws_y, r, ws_r = ops.stem_block(xd, w3d, b3d, w1d, b1d, GROUPS)
    torch.cuda.synchronize()
    dy, dr = float((y.cpu().double() - y_ref).abs().max()), float((r.cpu().double() - r_ref).abs().max())
    sy, sr = stats_error(ws_y, y, B), stats_error(ws_r, r, B)
    print("\nstem_block Cin %d B %d %dx%d: max|y - ref64| %.2e, max|r - ref64| %.2e (bar 5e-6); statistics %.2e, %.2e (bar 2e-6)" % (cin, B, H, W, dy, dr, sy, sr))
    assert dy <= 5e-6 and dr <= 5e-6
    assert sy <= 2e-6 and sr <= 2e-6
    # both maps are cf_conv2d_small_cin's bit for bit (the same fmaf chain per output; at six channels two rows share a packed instruction)
    assert torch.equal(r, ops.conv2d_small_cin(xd, w1d, b1d, None))
    assert torch.equal(y, ops.conv2d_small_cin(xd, w3d, b3d, None))
    # no bias
    y0, _, r0, _ = ops.stem_block(xd, w3d, None, w1d, None, GROUPS)
    assert float((y0.cpu().double() - (y_ref - b3.double()[None, :, None, None])).abs().max()) <= 5e-6
    assert float((r0.cpu().double() - (r_ref - b1.double()[None, :, None, None])).abs().max()) <= 5e-6


@pytest.mark.parametrize("cin", [1, 6])
def test_stem_block_keeps_samples_apart(dev, cin):
    """a NaN planted in sample 1 shows in sample 1's maps and statistics only"""
    from cineflow import ops
    B, H, W = 2, 20, 36
    x, w3, b3, w1, b1, _, _ = inputs(cin, B, H, W)
    xd, w3d, b3d, w1d, b1d = (t.to(dev) for t in (x, w3, b3, w1, b1))
    clean = ops.stem_block(xd, w3d, b3d, w1d, b1d, GROUPS)
    xn = xd.clone()
    xn[1, cin - 1, 7, 9] = float("nan")
    got = ops.stem_block(xn, w3d, b3d, w1d, b1d, GROUPS)
    for k in (0, 2):
        out_c, out_g, ws_g = clean[k], got[k], got[k + 1]
        assert torch.equal(out_c[0], out_g[0]) and torch.isnan(out_g[1]).any()
        assert torch.isfinite(ws_g[:2 * GROUPS]).all() and torch.isnan(ws_g[2 * GROUPS:]).all()
        assert stats_error(ws_g[:2 * GROUPS], out_g[:1], 1) <= 2e-6


def test_stem_block_probe_and_block_route(dev):
    """the probe declines what the kernel is not built for, and DoubleConv takes the one-launch route exactly when the probe accepts"""
    from cineflow import ops
    from cineflow.nn import DoubleConv
    from cineflow.weights import seeded_state_dict
    assert not ops.stem_block_ok(torch.empty(2, 2, 8, 8, device=dev), COUT, GROUPS)
    assert not ops.stem_block_ok(torch.empty(2, 6, 8, 8, device=dev), 60, GROUPS)
    with pytest.raises(RuntimeError):
        ops.stem_block(torch.zeros(1, 3, 8, 8, device=dev), torch.zeros(8, 3, 3, 3, device=dev), None, torch.zeros(8, 3, 1, 1, device=dev), None, 8)
    seen = []
    real = ops.stem_block
    ops.stem_block = lambda *a: (seen.append(a[0].shape[1]), real(*a))[1]
    try:
        for cin, stride, want in ((1, 1, True), (6, 1, True), (6, 2, False), (2, 1, False)):
            m = DoubleConv(cin, 16, True, stride)
            m.load_state_dict(seeded_state_dict(m.state_shapes(), 5), dev)
            n = len(seen)
            out = m(randn(2, cin, 16, 24, seed=9).to(dev))
            assert out.shape == (2, 16, 16 // stride, 24 // stride) and (len(seen) == n + 1) == want, (cin, stride)
    finally:
        ops.stem_block = real
