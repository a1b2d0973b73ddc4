"""Operator-level tables for the 3-D sliding window (cf_flip3d, cf_tta_accumulate_3d, cf_tile_accumulate_3d), the export resize
(cf_resize3d), cf_argmax_channels and cf_sample_points_2d, each launched on its own against the restatements of tests/_kernel_refs.py.
The whole-network tests reach these kernels only at 1e-4-class bars, where a swapped axis pair on a cubic patch hides behind the TTA
symmetry; here the extents are distinct and every mirroring is also checked on its own.

Bars.  flip3d: bit-identical to torch.flip.  tta_accumulate_3d: 1e-6 against the fp64 softmax (test_tta_and_tiles' bar for the 2-D twin);
with D = 1 bit-identical to ops.tta_accumulate (same formula, same order).  tile_accumulate_3d: bit-identical to fp32 slice adds (one
fp32 add per element and launch).  resize3d: order 0 identical, linear 2e-6 on [0, 1) data (test_export_resampling's bar).
sample_points: 2e-6 against fp32 F.grid_sample on the CPU (the warp family's bar), 1e-5 x max|field| against fp64.

argmax_channels and NaN: torch.argmax treats NaN as the maximum; the kernel scans with `v > best` from best = -inf, arg = 0, so a NaN
never wins and a pixel whose channels are all NaN (or all -inf) gives 0.  The NaN row asserts that documented rule (and that torch's
answer differs); everywhere else the kernel must equal torch.argmax, ties to the first index.

Measured on the MI355X (pytest -s prints one line per row: worst figure, bar, ratio):
  flip3d (40 rows), tile_accumulate_3d (4 rows), resize3d order 0, argmax_channels: identical
  tta_accumulate_3d: each mirroring alone 1.52e-7 (ratio 0.15), the eight at 1/8 2.12e-7 (0.21), 17 x 251 x 247 9.4e-8 (0.09)
  resize3d linear (75 rows): worst 1.31e-7 (3 x (5, 9, 8) -> (50, 90, 80)), ratio 0.066
  sample_points: 4.8e-7 against fp32 grid_sample (ratio 0.24), 3.1e-6 against fp64 (ratio 0.09 of 1e-5 x max|field|)
"""
import itertools

import pytest
import torch

from _kernel_refs import flip, ratio_line, resize_edge, sample_points, tile_add, tta_softmax

pytestmark = pytest.mark.gpu

FLAGS = list(itertools.product((0, 1), repeat=3))


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def maxdiff(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ flip3d
@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 7), (1, 1, 1, 1, 9), (1, 1, 9, 1, 1), (4, 2, 3), (2, 3, 17, 103, 101)])
def test_flip3d_table(dev, shape):
    from cineflow import ops
    x = randn(*shape, seed=len(shape) + shape[-1])
    x.view(-1)[0] = float("nan")
    x.view(-1)[-1] = -0.0
    xd = x.to(dev)
    print()
    for f in FLAGS:
        got = ops.flip3d(xd, *f)
        assert got.shape == x.shape
        nbad = int((bits(got) != bits(flip(x, f))).sum())
        ratio_line("flip3d %s flags %s: differing values" % (shape, f), float(nbad), 0)
        assert nbad == 0
    assert torch.equal(bits(xd), bits(x))                                # the source is left alone


# ------------------------------------------------------------------------------------------------ tta_accumulate_3d
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("dhw", [(3, 5, 4), (4, 4, 4), (1, 6, 7)])
def test_tta_accumulate_3d_table(dev, K, dhw):
    from cineflow import ops
    B = 2
    logits = 3.0 * randn(B, K, *dhw, seed=K + dhw[0])
    logits[1, :, 0, 1, 2] = torch.tensor([80.0, -80.0, 0.0, 1.0, -1.0])[:K]          # the max subtraction
    want = tta_softmax(logits)
    acc = torch.zeros(B, K, *dhw, device=dev)
    worst1 = 0.0
    for f in FLAGS:
        mirrored = flip(logits, f).contiguous().to(dev)
        ops.tta_accumulate_3d(mirrored, acc, *f, 0.125)
        one = ops.tta_accumulate_3d(mirrored, torch.zeros(B, K, *dhw, device=dev), *f, 1.0)   # each mirroring on its own: no symmetry to hide in
        worst1 = max(worst1, maxdiff(one, want))
    print()
    ratio_line("tta_accumulate_3d K=%d %s: each mirroring alone" % (K, dhw), worst1, 1e-6)
    ratio_line("tta_accumulate_3d K=%d %s: the eight at weight 1/8" % (K, dhw), maxdiff(acc, want), 1e-6)
    assert worst1 <= 1e-6 and maxdiff(acc, want) <= 1e-6
    if K > 1:                                                            # the rows can tell a wrong mirroring from a right one
        wrong = ops.tta_accumulate_3d(flip(logits, (0, 1, 0)).contiguous().to(dev), torch.zeros(B, K, *dhw, device=dev), 0, 0, 1, 1.0)
        assert maxdiff(wrong, want) > 1e-3


def test_tta_accumulate_3d_one_slice_is_the_2d_kernel(dev):
    from cineflow import ops
    B, K, H, W = 2, 4, 12, 10
    logits = 4.0 * randn(B, K, H, W, seed=78)
    acc2, acc3 = (0.1 * randn(B, K, H, W, seed=79)).to(dev), (0.1 * randn(B, K, H, W, seed=79)).to(dev)[:, :, None].contiguous()
    for fh, fw in itertools.product((0, 1), repeat=2):
        ld = flip(logits, (fh, fw)).contiguous().to(dev)
        ops.tta_accumulate(ld, acc2, fh, fw, 0.25)
        ops.tta_accumulate_3d(ld[:, :, None].contiguous(), acc3, 0, fh, fw, 0.25)
        assert torch.equal(bits(acc3[:, :, 0]), bits(acc2)), (fh, fw)
    assert maxdiff(acc2 - (0.1 * randn(B, K, H, W, seed=79)).to(dev), tta_softmax(logits)) <= 1e-6


def test_tta_accumulate_3d_second_trip(dev):
    from cineflow import ops
    logits = 3.0 * randn(1, 2, 17, 251, 247, seed=5)                     # 1,053,949 voxels
    f = (1, 0, 1)
    got = ops.tta_accumulate_3d(flip(logits, f).contiguous().to(dev), torch.zeros(1, 2, 17, 251, 247, device=dev), *f, 1.0)
    worst = maxdiff(got, tta_softmax(logits))
    print()
    ratio_line("tta_accumulate_3d 17 x 251 x 247, flags (1, 0, 1)", worst, 1e-6)
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------ tile_accumulate_3d
@pytest.mark.parametrize("with_gauss", [False, True])
@pytest.mark.parametrize("K", [1, 3])
def test_tile_accumulate_3d_table(dev, K, with_gauss):
    from cineflow import ops
    X, Y, Z, patch = 11, 13, 9, (6, 7, 5)
    corners = [(2, 3, 1), (X - patch[0], Y - patch[1], Z - patch[2]), (0, 0, 0)]       # overlapping; one flush with the far corner
    agg0, cnt0 = randn(K, X, Y, Z, seed=1), randn(K, X, Y, Z, seed=2) + 9.0              # sentinels: what no tile covers must stay as it is
    agg, cnt = agg0.clone().to(dev), cnt0.clone().to(dev)
    ra, rc = agg0.clone(), cnt0.clone()
    g = (torch.rand(*patch, generator=torch.Generator().manual_seed(3)) + 0.1) if with_gauss else None
    covered = torch.zeros(X, Y, Z, dtype=torch.bool)
    for j, c in enumerate(corners):
        pred = torch.softmax(randn(K + 1, *patch, seed=10 + j), 0)[:K].contiguous() * (g if with_gauss else 1.0)
        ops.tile_accumulate_3d(pred.to(dev), None if g is None else g.to(dev), agg, cnt, *c)
        tile_add(ra, rc, pred, g, c)
        covered[tuple(slice(a, a + p) for a, p in zip(c, patch))] = True
    na, nc = int((bits(agg) != bits(ra)).sum()), int((bits(cnt) != bits(rc)).sum())
    print()
    ratio_line("tile_accumulate_3d K=%d gauss=%s: differing agg / cnt values" % (K, with_gauss), float(na + nc), 0)
    assert na == 0 and nc == 0
    assert not covered.all() and torch.equal(bits(agg.cpu()[:, ~covered]), bits(agg0[:, ~covered])) and torch.equal(bits(cnt.cpu()[:, ~covered]), bits(cnt0[:, ~covered]))
    from cineflow._lib import CineflowError
    with pytest.raises(CineflowError):                                   # a tile past the far corner is refused on the host
        ops.tile_accumulate_3d(pred.to(dev), None, agg, cnt, X - patch[0] + 1, 0, 0)


# ------------------------------------------------------------------------------------------------ resize3d
RESIZE_SHAPES = [((5, 20, 24), (8, 31, 17)), ((5, 20, 24), (5, 20, 24)), ((8, 20, 24), (4, 10, 12)),          # up / down, identity, half-way samples
                 ((1, 6, 7), (3, 9, 4)), ((6, 1, 7), (3, 9, 4)), ((6, 7, 1), (3, 9, 4)), ((6, 7, 5), (1, 1, 1)), ((1, 1, 1), (3, 2, 5)),
                 ((3, 4, 5), (30, 40, 50))]


@pytest.mark.parametrize("shape,new", RESIZE_SHAPES)
def test_resize3d_table(dev, shape, new):
    from cineflow import ops
    x = torch.rand(2, *shape, generator=torch.Generator().manual_seed(shape[0] * 100 + new[2]))
    xd = x.to(dev)
    print()
    for lin in FLAGS:
        want = resize_edge(x.numpy(), new, lin)
        got = ops.resize3d(xd, new, lin)
        assert tuple(got.shape) == (2,) + tuple(new)
        bar = 2e-6 if any(lin) else 0.0
        worst = maxdiff(got, want)
        ratio_line("resize3d %s -> %s linear %s" % (shape, new, lin), worst, bar)
        assert worst <= bar
        if shape == new:
            assert torch.equal(bits(got), bits(x))


def test_resize3d_second_trip(dev):
    from cineflow import ops
    x = torch.rand(3, 5, 9, 8, generator=torch.Generator().manual_seed(9))
    new = (50, 90, 80)                                                   # 3 x 360,000 outputs, every axis up by 10
    print()
    for lin in ((1, 1, 1), (0, 0, 0), (0, 1, 0)):
        worst = maxdiff(ops.resize3d(x.to(dev), new, lin), resize_edge(x.numpy(), new, lin))
        ratio_line("resize3d 3 x (5, 9, 8) -> (50, 90, 80) linear %s" % (lin,), worst, 2e-6 if any(lin) else 0.0)
        assert worst <= (2e-6 if any(lin) else 0.0)


# ------------------------------------------------------------------------------------------------ argmax_channels
def test_argmax_channels_table(dev):
    from cineflow import ops
    x = randn(2, 5, 7, 9, seed=4)
    x[0, :, 0, 0] = 1.5                                                  # a five-way tie: the first index
    x[0, 1, 0, 1] = x[0, 3, 0, 1] = 9.0
    x[1, :, 2, 2] = float("-inf")
    x[1, 4, 3, 3] = float("inf")
    assert torch.equal(ops.argmax_channels(x.to(dev)).cpu().long(), x.argmax(1))
    assert int(x.argmax(1)[0, 0, 0]) == 0 and int(x.argmax(1)[0, 0, 1]) == 1
    one = randn(3, 1, 4, 5, 6, seed=5)                                   # K = 1, and a 3-D map
    assert torch.equal(ops.argmax_channels(one.to(dev)).cpu().long(), torch.zeros(3, 4, 5, 6, dtype=torch.long))
    big = randn(1, 3, 17, 251, 247, seed=6)                              # > 2^20 pixels
    assert torch.equal(ops.argmax_channels(big.to(dev)).cpu().long(), big.argmax(1))
    # NaN: torch.argmax lets it win, the kernel's `v > best` scan never does (see the module docstring)
    n = randn(1, 3, 2, 4, seed=7)
    n[0, 0, 0, 0] = n[0, 2, 0, 1] = n[0, 1, 1, 2] = float("nan")
    n[0, :, 1, 3] = float("nan")
    rule = torch.where(torch.isnan(n), torch.full_like(n, float("-inf")), n).argmax(1)
    rule[0, 1, 3] = 0
    assert torch.equal(ops.argmax_channels(n.to(dev)).cpu().long(), rule)
    assert not torch.equal(n.argmax(1), rule)


# ------------------------------------------------------------------------------------------------ sample_points
def _points(B, P, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.stack([torch.rand(B, P, generator=g) * (W + 1) - 1.0, torch.rand(B, P, generator=g) * (H + 1) - 1.0], 1)
    special = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [3.0, 2.0], [W - 1.0, 1.0], [2.0, H - 1.0],            # on pixels; the last row / column exactly
                            [-0.5, 2.0], [W - 0.5, 2.0], [3.0, -0.5], [3.0, H - 0.5], [-0.5, -0.5], [W - 0.5, H - 0.5],   # half a pixel outside, each side
                            [-1.0, 1.0], [float(W), 1.0], [1e4, 1.0], [1.0, -1e4], [-3e7, 3e7], [2.25, 4.75]])            # on the zero ring and far outside
    k = min(P, len(special))
    if P > 1:
        pts[:, :, :k] = special[:k].t()[None]
        pts[:, :, P - k:] = special[:k].t()[None].flip(-1)
    return pts


@pytest.mark.parametrize("B,C,H,W,P", [(1, 1, 9, 13, 1), (2, 3, 9, 13, 257), (2, 3, 13, 9, 257), (1, 2, 2, 2, 40), (2, 8, 9, 13, 66000)])
def test_sample_points_table(dev, B, C, H, W, P):
    from cineflow import ops
    field = randn(B, C, H, W, seed=H * W + P)
    pts = _points(B, P, H, W, seed=P)
    got = ops.sample_points(field.to(dev), pts.to(dev))
    want32, want64 = sample_points(field, pts), sample_points(field.double(), pts.double())
    fmax = float(field.abs().max())
    print()
    ratio_line("sample_points %s P=%d: vs fp32 grid_sample" % ((B, C, H, W), P), maxdiff(got, want32), 2e-6)
    ratio_line("sample_points %s P=%d: vs fp64 grid_sample" % ((B, C, H, W), P), maxdiff(got, want64), 1e-5 * fmax)
    assert tuple(got.shape) == (B, C, P) and maxdiff(got, want32) <= 2e-6 and maxdiff(got, want64) <= 1e-5 * fmax
    if P >= 17:                                                          # the rows mean what they say
        w = want64[0, 0]
        assert abs(float(w[0] - field[0, 0, 0, 0])) < 1e-12 and abs(float(w[1] - field[0, 0, H - 1, W - 1])) < 1e-12
        assert abs(float(w[5] - 0.5 * field[0, 0, 2 % H, 0])) < 1e-12 or H <= 2
        assert float(w[11:16].abs().max()) < 1e-12
