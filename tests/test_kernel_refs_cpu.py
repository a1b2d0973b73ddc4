"""CPU checks of tests/_kernel_refs.py: every restatement the GPU operator tables use is pinned to the oracle (which the golden vectors
pin to the reference) or to the scipy call that defines it, so that a restatement and the HIP kernel it judges cannot be wrong together."""
import numpy as np
import pytest
import torch

import _kernel_refs as R


def test_fill_holes_equals_oracle_on_fixture(golden):
    from oracle import preprocess as OP
    g = golden("preprocess_crop")
    assert np.array_equal(R.nonzero_fill_holes(g["data"]), OP.create_nonzero_mask(g["data"]))
    assert np.array_equal(R.nonzero_fill_holes(g["data"]), g["mask"])
    assert np.array_equal(R.nonzero_fill_holes(g["data"][:, 4]), OP.create_nonzero_mask(g["data"][:, 4]))
    assert R.bbox(g["mask"]) == g["bbox"].tolist() == OP.get_bbox_from_mask(g["mask"])
    with pytest.raises(ValueError):
        R.bbox(np.zeros((2, 3, 4), bool))


def test_fill_holes_scipy_facts():
    """the two facts of scipy.ndimage.binary_fill_holes the device has to reproduce"""
    ring = np.zeros((9, 9), np.float32)
    ring[2:7, 2:7] = 1
    ring[3:6, 3:6] = 0
    # a one-slice 3-D array fills nothing (every voxel lies on a z face); the same slice as a 2-D array fills
    assert np.array_equal(R.nonzero_fill_holes(ring[None, None]), ring[None] != 0)
    assert R.nonzero_fill_holes(ring[None]).sum() == 25
    # a background pocket that reaches the border only through diagonal steps is a hole
    diag = np.ones((6, 6), np.float32)
    for i in range(4):
        diag[i, i] = 0
    want = np.ones((6, 6), bool)
    want[0, 0] = False                                 # the corner voxel is border background; the chain behind it is filled
    assert np.array_equal(R.nonzero_fill_holes(diag[None]), want)
    # NaN counts as non-zero, -0.0 does not
    x = np.zeros((2, 1, 2, 2), np.float32)
    x[0, 0, 0, 0], x[1, 0, 1, 1] = np.nan, -0.0
    assert R.nonzero_fill_holes(x).tolist() == [[[True, False], [False, False]]]


def test_seg_outside_mask_equals_oracle(golden):
    from oracle import preprocess as OP
    g = golden("preprocess_crop")
    rng = np.random.default_rng(5)
    seg = rng.integers(0, 3, (2,) + g["data"].shape[1:]).astype(np.float32)
    d, s, bb = OP.crop_to_nonzero(g["data"].copy(), seg.copy(), 5)
    sl = tuple(slice(*b) for b in bb)
    assert np.array_equal(R.seg_outside_mask(seg[(slice(None),) + sl], g["mask"][sl], 5), s)


def test_cubic_axis_composes_to_oracle_resize():
    from oracle import preprocess as OP
    x = np.random.default_rng(0).normal(size=(6, 11, 9))
    new = (9, 7, 23)
    y = x
    for a, m in enumerate(new):
        y = R.cubic_axis(y, a, m)
    ref = OP.resize(x, new, order=3, clip=False)
    assert y.shape == ref.shape and float(np.abs(y - ref).max()) <= 1e-12 * np.abs(x).max()
    mn, mx = R.slab_minmax(x[None, None].reshape(1, 1, 1, -1))
    assert np.array_equal(R.slab_clip_f32(y[None, None].reshape(1, 1, 1, -1), mn, mx).reshape(new),
                          np.clip(ref, x.min(), x.max()).astype(np.float32))


@pytest.mark.parametrize("ws,shift,H,W,heads,hd", [(7, 3, 14, 21, 2, 4), (4, 0, 8, 12, 3, 5)])
def test_window_attention_equals_oracle(ws, shift, H, W, heads, hd):
    """against oracle.mtl's SwinCrossAttention with identity projections and LayerNorm bypassed: its CrossAttention (relative_position_index
    buffer, bias table) under its own attn_mask buffer, roll, window_partition and window_reverse"""
    from oracle import mtl as OM
    C, B = heads * hd, 2
    g = torch.Generator().manual_seed(ws)
    q, k, v = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) for _ in range(3))
    table = 0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=g, dtype=torch.float64)
    sw = OM.SwinCrossAttention(C, (H, W), heads, ws, shift).double()
    assert sw.window_size == ws and sw.shift_size == shift and (sw.attn_mask is not None) == (shift > 0)
    ca = sw.cross_attn
    with torch.no_grad():
        ca.relative_position_bias_table.copy_(table)
        ca.proj.weight.copy_(torch.eye(C)), ca.proj.bias.zero_()

    class Pick(torch.nn.Module):                       # the projections bypassed: q | k ride in the rescaler tokens, v in the rescaled ones
        def __init__(self, parts):
            super().__init__()
            self.parts = parts

        def forward(self, x):
            B_, N, Ct = x.shape
            return tuple(x[..., i * C:(i + 1) * C].reshape(B_, N, heads, hd).permute(0, 2, 1, 3) if i is not None else None for i in self.parts)

    ca.get_qkv_object_rescaled, ca.get_qkv_object_rescaler = Pick((None, None, 0)), Pick((0, 1, None))

    def windows(t):                                    # BeforeCrossAttention without its LayerNorm
        Bc, Ct = t.shape[:2]
        t = t.permute(0, 2, 3, 1)
        if shift:
            t = torch.roll(t, (-shift, -shift), (1, 2))
        return OM.window_partition(t.contiguous(), ws).view(-1, ws * ws, Ct)

    with torch.no_grad():
        a = ca(windows(v), windows(torch.cat([q, k], 1)), mask=sw.attn_mask)
    x = OM.window_reverse(a.view(-1, ws, ws, C), ws, H, W)
    if shift:
        x = torch.roll(x, (shift, shift), (1, 2))
    ref = x.permute(0, 3, 1, 2)
    out = R.window_attention(q, k, v, table, heads, ws, shift)
    assert float((out - ref).abs().max()) <= 1e-12
    if shift:                                          # and the mask term matters at this size
        assert float((R.window_attention(q, k, v, table, heads, ws, shift, mask=False) - ref).abs().max()) > 1e-3


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape,new", [((5, 20, 24), (8, 31, 17)), ((4, 9, 6), (2, 90, 7)), ((1, 7, 8), (3, 7, 20))])
def test_resize_equals_oracle(order, shape, new):
    from oracle import ops as OO
    x = np.random.default_rng(2).random((2,) + shape)
    ref = OO.resample_data_or_seg(x, new, False, None, order, False, 0)
    out = R.resize_edge(x, new, [order] * 3)
    assert out.shape == ref.shape
    assert float(np.abs(out - ref).max()) <= (0 if order == 0 else 1e-14)


def test_small_restatements():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 4, 5, 6, generator=g)
    assert torch.equal(R.flip(x, (1, 0, 1)), torch.flip(x, (2, 4))) and torch.equal(R.flip(x, (0, 0, 0)), x)
    assert torch.equal(R.flip(x[0, 0], (0, 1)), torch.flip(x[0, 0], (2,)))
    # mirrored passes over mirrored logits, mirrored back, average to the softmax of the un-mirrored logits
    acc = sum(R.flip(torch.softmax(R.flip(x, f).double(), 1), f) for f in ((0, 0, 0), (1, 1, 0), (0, 1, 1))) / 3
    assert float((acc - R.tta_softmax(x)).abs().max()) <= 1e-15
    agg, cnt = torch.zeros(3, 6, 7, 8), torch.zeros(3, 6, 7, 8)
    R.tile_add(agg, cnt, x[0, :, :, :, :4], None, (2, 2, 4))
    assert float(cnt.sum()) == 3 * 4 * 5 * 4 and torch.equal(agg[:, 2:, 2:, 4:], x[0, :, :, :, :4]) and float(agg[:, :2].abs().sum()) == 0
    n, s1, s2, sa = R.masked_moments(np.array([1, 2, 3, 4], np.float32), seg=np.array([0, 0, -1, 0]), lo=1, hi=4)
    assert (n, s1, s2, sa) == (1, 2.0, 4.0, 2.0)
    y = R.normalize_f32(np.array([-5, 0, 5], np.float32), 1, 2, clip=(-2, 2), seg=np.array([0, -1, 0]), zero_outside=True)
    assert y.tolist() == [-1.5, 0.0, 0.5] and y.dtype == np.float32


def test_sample_points_equals_oracle_strain(golden):
    g = golden("strain")
    field, pts = torch.from_numpy(g["stc_field"]), torch.from_numpy(g["stc_pts"])
    B, P = pts.shape[0], pts.shape[-1] if pts.dim() == 3 else pts.numel() // (2 * pts.shape[0])
    out = R.sample_points(field, pts.reshape(B, 2, P))
    assert float((out - torch.from_numpy(g["stc_out"])[:, :, 0]).abs().max()) <= 2e-6


@pytest.mark.parametrize("B,C,H,W,levels", [(2, 32, 16, 20, 4), (1, 24, 8, 24, 3), (2, 16, 16, 32, 4)])
def test_allpairs_pyramid_equals_oracle(B, C, H, W, levels):
    """the fp64 restatement against oracle.ops.corr_allpairs / corr_pyramid run in float64 (rounding only) and in their own float32 (the
    fp32 matmul's error on unit-normal features: sqrt(C) x 2^-24 x a few), at a size whose levels pool 5 -> 2"""
    from oracle import ops as OO
    g = torch.Generator().manual_seed(H + W)
    f1, f2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    out = R.allpairs_pyramid(f1, f2, levels)
    ref64 = OO.corr_pyramid(OO.corr_allpairs(f1.double(), f2.double()), levels)
    ref32 = OO.corr_pyramid(OO.corr_allpairs(f1, f2), levels)
    assert len(out) == len(ref64) == levels
    for l in range(levels):
        assert out[l].dtype == torch.float64 and out[l].shape == ref64[l].shape == (B, H * W, H >> l, W >> l)
        assert float((out[l] - ref64[l]).abs().max()) <= 1e-13
        assert float((out[l] - ref32[l].double()).abs().max()) <= 5e-6


def _inside(H, W, radius, stride):
    """[(2r+1)^2, H, W] bool: the displacement stays inside the map"""
    D = 2 * radius + 1
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    m = torch.zeros(D * D, H, W, dtype=torch.bool)
    for i in range(D):
        for j in range(D):
            yy, xx = y + (i - radius) * stride, x + (j - radius) * stride
            m[i * D + j] = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    return m


@pytest.mark.parametrize("B,C,H,W,radius,stride", [(1, 16, 8, 64, 4, 1), (2, 256, 8, 64, 4, 1), (2, 128, 16, 64, 4, 2), (3, 64, 32, 64, 4, 4),
                                                  (2, 5, 7, 9, 4, 2), (1, 4, 6, 10, 8, 1), (1, 4, 6, 10, 0, 1), (1, 4, 6, 10, 4, 3)])
def test_corr_volume_refs_equal_oracle_and_resolve(B, C, H, W, radius, stride):
    """corr_volume_refs against oracle.ops.corr_volume, and what the two bars of test_gpu_corr_volume_routes.py resolve, as multiples of
    SPLIT_BAR x A = 2^-18 A (maximum over the volume; unit-normal operands):
        (B, C, H, W, S)       hi x hi only   lo x hi of 8 channels   last channel   lo x lo   y4 - true
        (1, 16, 8, 64, 1)        124             68.4                 1.4e5          0.023     0.035
        (2, 256, 8, 64, 1)        31.8            6.35                1.5e4          0.005     0.007
        (2, 128, 16, 64, 2)       52.4           12.7                 3.6e4          0.008     0.010
        (3, 64, 32, 64, 4)        72.9           28.7                 6.2e4          0.012     0.016
    lo x lo is below the bar: it cannot be resolved and is not asserted.  The split's own truncation y4 - true is bounded by reasoning:
    |x - xh - xl| <= 2^-22 |x| (two roundings to 11 bits), so |y4 - true| <= (2 x 2^-22 + 2^-44) A1 < 0.13 x 2^-18 A."""
    from oracle import ops as OO
    from _split_exact import SPLIT_BAR
    cur, prev = (torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(s)) for s in (C + H, C + W + 1))
    r = R.corr_volume_refs(cur, prev, radius, stride)
    D = 2 * radius + 1
    for k, v in r.items():
        assert v.dtype == torch.float64 and v.shape == (B, D * D, H, W), k
    ref64 = OO.corr_volume(cur.double(), prev.double(), radius, stride)
    assert float((r["true"] - ref64).abs().max()) <= 1e-14
    inside = _inside(H, W, radius, stride)[None].expand(B, -1, -1, -1)
    assert torch.equal(r["A"] == 0, ~inside) and torch.equal(r["A1"] == 0, ~inside)
    for k in ("true", "y4", "y1", "d_last", "d_lohi8"):
        assert bool((r[k][~inside] == 0).all()), k
    bar = (SPLIT_BAR * r["A"])[inside]
    of = lambda d: float((d[inside].abs() / bar).max())
    assert float((r["A"] - r["A1"]).abs().max()) <= 2.0 ** -10 * float(r["A1"].max()) and bool((r["A"] >= r["A1"] * (1 - 2.0 ** -20)).all())
    split_err = of(r["y4"] - r["true"])
    hh, lohi8, last = of(r["y1"] - r["y4"]), of(r["d_lohi8"]), of(r["d_last"])
    print("\n  %s: hi x hi only %.3g, lo x hi of 8 channels %.3g, last channel %.3g, y4 - true %.3g (x 2^-18 A)" % ((B, C, H, W, stride), hh, lohi8, last, split_err))
    assert split_err <= 0.13, split_err
    assert hh > 1 and lohi8 > 1 and last > 1, (hh, lohi8, last)                       # the split-exact bar resolves each of them
    # the fp32 bar of the two fp32 kernels: any C-term fp32 sum, the rounding of 1 / C and of the final product -> (C + 3) 2^-24 A1;
    # the oracle's own float32 run meets it, and taking one channel away does not
    bar32 = ((C + 3) * 2.0 ** -24 * r["A1"])[inside]
    own = float(((OO.corr_volume(cur, prev, radius, stride).double() - r["true"])[inside].abs() / bar32).max())
    assert own <= 1.0, own
    assert float((r["d_last"][inside].abs() / bar32).max()) > 1
