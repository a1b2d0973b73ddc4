"""Pins tests/_tap_chain.py, the numpy float32 restatement of the bilinear-tap arithmetic of csrc/common.h that test_gpu_tap_chains.py holds
the kernels to with `==` (no GPU here).

  goldens and oracle   the chain has the oracle's standing: the reference's golden vectors and oracle.ops at the bars of test_gpu_ops.py
                       (warp 2e-6, vecint 1e-5, 3-D 5e-5, lookups 3e-5, labels equal on every pixel)
  hand-worked cases    integer shifts copy and zero-fill exactly; zero flow is the identity where the normalisation round-trips; a flow of
                       exactly k + 0.5 between two labels gives the lower class; NaN / +inf / -inf flows give NaN (2-D), 0 (3-D), class 0
                       (labels); finite far flows give 0
  resolving power      on the inputs of the GPU rows (the table at the end of _tap_chain.py) every variant differs from the chain
  fp64 sanity          warp2d within 8 x 2^-24 x (|a| w00 + |b| w01 + |c| w10 + |d| w11) of the same taps and weights in float64

One variant cannot be resolved on any output.  `corner_weights` forms ey as (yf + 1) - y instead of 1 - (y - yf).  y - yf is exact for
y >= 0 and for y < -1 (a multiple of ulp(y) below 1), and yf + 1 is exact below 2^24, so both forms round the same real number: they can
only differ for y in (-1, 0), where 1 + y may round, and from 2^24 up, where yf + 1 does.  In both places ey weighs row y0 = -1 (or a row
past 2^24), which is outside every image: the tap is invalid, its value is 0 and 0 x ey is +0 either way.  The same holds for ex.  So
that variant is pinned where it does show, on the weights (test_corner_weights_show_on_invalid_taps_only), and the rows' outputs are
shown to be unable to see it rather than claimed to.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tap_chain as TC
from _kernel_refs import allpairs_pyramid

F32, F64 = np.float32, np.float64
T = torch.from_numpy


def maxdiff(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b.numpy() if isinstance(b, torch.Tensor) else b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max())


def differing(a, b):
    """elements whose values differ; two NaNs count as equal"""
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()) if a.dtype == F32 else int((a != b).sum())


def cpu_pyramid(f1, f2, levels):
    """the fp64 pyramid rounded to fp32 (the GPU rows look up the device's own pyramid of the same features)"""
    return [p.float().numpy() for p in allpairs_pyramid(T(f1), T(f2), levels)]


# ===================================================================================================== goldens and oracle
@pytest.mark.parametrize("tag", ["32", "40x24"])
def test_golden_2d(golden, tag):
    from oracle import ops as OO
    g = golden("warp_" + tag)
    flow, src = g["flow"], g["src"]
    out, vi = TC.warp2d(flow, src), TC.vecint2d(flow, 7)
    assert out.dtype == F32 and vi.dtype == F32
    assert maxdiff(out, g["warped"]) <= 2e-6 and maxdiff(out, OO.warp_bilinear(T(flow).clone(), T(src))) <= 2e-6
    assert maxdiff(vi, g["vecint"]) <= 1e-5 and maxdiff(vi, OO.vecint(T(flow).clone(), 7)) <= 1e-5


def test_golden_3d(golden):
    from oracle import ops as OO
    g = golden("warp_3d")
    flow, src = g["flow"], g["src"]
    out, vi = TC.warp3d(flow, src), TC.vecint3d(flow, 7)
    assert maxdiff(out, g["warped"]) <= 2e-6 and maxdiff(out, OO.warp_bilinear(T(flow).clone(), T(src))) <= 2e-6
    assert maxdiff(vi, g["vecint"]) <= 1e-5 and maxdiff(vi, OO.vecint(T(flow).clone(), 7)) <= 1e-5


def test_golden_256(golden):
    from oracle import ops as OO
    g = golden("warp_256")
    src = torch.randn(1, 4, 256, 256, generator=torch.Generator().manual_seed(13))       # the inputs of test_warp_256_golden_and_properties
    flow = F.avg_pool2d(torch.randn(1, 2, 288, 288, generator=torch.Generator().manual_seed(12)), 33, stride=1) * 120.0
    out = TC.warp2d(flow, src)
    assert maxdiff(out[:, :, :16, :16], g["warped_corner"]) <= 2e-6
    assert maxdiff(out[:, :, 120:136, 120:136], g["warped_center"]) <= 2e-6
    assert abs(float(out.astype(F64).sum()) - float(g["checksum"])) < 1e-2
    assert maxdiff(out, OO.warp_bilinear(flow.clone(), src)) <= 2e-6


def test_golden_labels(golden):
    g = golden("warp_labels")
    out = TC.warp_labels2d(g["flow"], g["labels"][:, 0].astype(np.uint8), 4)
    assert out.dtype == np.uint8 and np.array_equal(out, g["registered"][:, :, 0].astype(np.uint8))


def test_oracle_3d():
    from oracle import ops as OO
    flows, src = TC.warp3d_inputs()
    assert src.shape == (2, 2, 5, 9, 7)
    assert maxdiff(TC.warp3d(flows["normal2"], src), OO.warp_bilinear(T(flows["normal2"]).clone(), T(src))) <= 5e-5


@pytest.mark.parametrize("name", list(TC.LOOKUP_ROWS))
def test_oracle_lookup(name):
    from oracle import ops as OO
    levels, radius = TC.LOOKUP_ROWS[name][4:6]
    f1, f2, coords = TC.lookup_row_inputs(name)
    pyr = cpu_pyramid(f1, f2, levels)
    out = TC.corr_lookup(pyr, coords, radius)
    assert out.dtype == F32
    assert maxdiff(out, OO.corr_lookup([T(p) for p in pyr], T(coords), radius)) <= 3e-5


def test_oracle_sample_points_and_memory_input():
    """sample_points is grid_sample at the normalised points; memory_input is cat(x0, xt, cum, x0 - reg, reg): the bars of the 2-D warp"""
    from oracle import ops as OO
    field, pts = TC.sample_points_inputs()
    H, W = field.shape[2:]
    ok = np.isfinite(pts).all(1) & (np.abs(pts) < 1e5).all(1)                              # [B, P]
    grid = torch.stack([2 * (T(pts[:, 0]) / (W - 1) - 0.5), 2 * (T(pts[:, 1]) / (H - 1) - 0.5)], -1)[:, None]
    ref = F.grid_sample(T(field), grid, align_corners=True)[:, :, 0].numpy()
    out = TC.sample_points(field, pts)
    sel = np.broadcast_to(ok[:, None, :], out.shape)
    assert maxdiff(out[sel], ref[sel]) <= 2e-6
    x0, xt, flows = TC.memory_row_inputs("3x21x30")
    cum = flows["normal3"]
    reg = OO.warp_bilinear(T(cum).clone(), T(xt))
    assert maxdiff(TC.memory_input(x0, xt, cum), torch.cat([T(x0), T(xt), T(cum), T(x0) - reg, reg], 1)) <= 2e-6


# ===================================================================================================== hand-worked cases
def test_integer_shift_copies_and_zero_fills():
    """at sizes whose normalisation round-trips (size - 1 a power of two); elsewhere the position is an ulp off the pixel, as in the reference"""
    H, W = 17, 33
    src = TC.randn(2, 3, H, W, seed=1)
    flow = np.zeros((2, 2, H, W), dtype=F32)
    flow[:, 0], flow[:, 1] = 5.0, -7.0
    want = np.zeros_like(src)
    want[:, :, :H - 5, 7:] = src[:, :, 5:, :W - 7]
    out = TC.warp2d(flow, src)
    assert np.array_equal(out, want) and not np.signbit(out[want == 0]).any()
    D = 5
    src3 = TC.randn(1, 2, D, 9, 5, seed=2)
    flow3 = np.zeros((1, 3, D, 9, 5), dtype=F32)
    flow3[:, 0], flow3[:, 1], flow3[:, 2] = 2.0, -3.0, 1.0
    want3 = np.zeros_like(src3)
    want3[:, :, :D - 2, 3:, :4] = src3[:, :, 2:, :6, 1:]
    assert np.array_equal(TC.warp3d(flow3, src3), want3)


@pytest.mark.parametrize("H,W", [(17, 9), (5, 33), (2, 3)])
def test_zero_flow_is_the_identity_where_the_normalisation_round_trips(H, W):
    """size - 1 a power of two: i / (S - 1), - 0.5, x 2, + 1, / 2 and x (S - 1) are all exact"""
    assert all((s - 1) & (s - 2) == 0 for s in (H, W))
    idx = np.arange(H, dtype=F32)
    assert np.array_equal(TC.st_coord(idx, np.zeros(H, dtype=F32), H - 1), idx)
    src = TC.randn(2, 2, H, W, seed=3)
    zero = np.zeros((2, 2, H, W), dtype=F32)
    assert np.array_equal(TC.warp2d(zero, src), src)
    assert np.array_equal(TC.memory_input(src[:, :1], src[:, 1:], zero)[:, 5], src[:, 1])
    lab = TC.rand_labels(2, H, W, K=4, seed=4)
    assert np.array_equal(TC.warp_labels2d(zero[None], lab, 4)[0], lab)
    src3 = TC.randn(1, 2, 3, H, W, seed=5)
    assert np.array_equal(TC.warp3d(np.zeros((1, 3, 3, H, W), dtype=F32), src3), src3)


def test_half_pixel_between_two_labels_gives_the_lower_class():
    H, W = 9, 17
    lab = np.zeros((1, H, W), dtype=np.uint8)
    lab[0, 4:] = 3                                       # rows 0..3 class 0, rows 4.. class 3; lab[0, :, 8:] untouched
    lab[0, :, 12:] = np.where(lab[0, :, 12:] == 0, 2, 3)
    flow = np.zeros((1, 1, 2, H, W), dtype=F32)
    flow[0, 0, 0, 3] = 0.5                               # row 3 samples exactly between rows 3 and 4: 0.5 / 0.5
    flow[0, 0, 0, 1] = 2.5                               # row 1 as well (k = 2)
    out = TC.warp_labels2d(flow, lab, 4)[0, 0]
    assert (out[3, :12] == 0).all() and (out[1, :12] == 0).all() and (out[3, 12:] == 2).all() and (out[1, 12:] == 2).all()
    tie = TC.warp_labels2d(flow, lab, 4, variant="last_tie")[0, 0]
    assert (tie[3] == 3).all() and (tie[1] == 3).all()
    flow[0, 0, 0, 3] = F32(0.5) + F32(2.0 ** -20)        # four ulps of 3.5 towards row 4: the higher class
    assert (TC.warp_labels2d(flow, lab, 4)[0, 0, 3] == 3).all()


def test_nonfinite_flows():
    B, C, H, W = 2, 3, 17, 24
    flows, src = TC.warp_row_inputs("v4 2x3x17x24")
    clean, flow = TC.warp2d(flows["normal3"], src), flows["nonfinite"]
    out = TC.warp2d(flow, src)
    planted = np.zeros((B, C, H, W), dtype=bool)
    for _, i, j in TC.nonfinite_pixels(H, W):
        planted[0, :, i, j] = True
    assert planted.sum() == 6 * C and np.isnan(out[planted]).all() and np.array_equal(out[~planted], clean[~planted])
    x0, xt = src[:, :1], src[:, 1:2]
    mem = TC.memory_input(x0, xt, flow)
    assert np.isnan(mem[:, 4:][planted[:, :2]]).all() and not np.isnan(mem[:, 4:][~planted[:, :2]]).any()
    assert np.array_equal(mem[:, :2], src[:, :2]) and np.array_equal(mem[:, 2:4], flow, equal_nan=True)
    lab = TC.rand_labels(B, H, W, K=4, seed=6) | 1       # no class 0 in the map: class 0 can only come from "nothing sampled"
    reg = TC.warp_labels2d(flow[None], lab, 4)[0]
    assert (reg[planted[:, 0]] == 0).all()
    assert (TC.warp_labels2d(flow[None], lab, 4, variant="last_tie")[0][planted[:, 0]] == 3).all()
    flows3, src3 = TC.warp3d_inputs()
    out3 = TC.warp3d(flows3["nonfinite"], src3)
    assert not np.isnan(out3).any()
    for z, y, x in TC.nonfinite_voxels():
        assert (out3[0, :, z, y, x] == 0).all() and not np.signbit(out3[0, :, z, y, x]).any()
    field, pts = TC.sample_points_inputs()
    sp = TC.sample_points(field, pts)
    bad = ~np.isfinite(pts).all(1)
    assert bad.sum() == 6 and np.isnan(sp[np.broadcast_to(bad[:, None], sp.shape)]).all() and not np.isnan(sp[np.broadcast_to(~bad[:, None], sp.shape)]).any()


@pytest.mark.parametrize("far", TC.FAR[:3])
def test_far_finite_flows_give_zero(far):
    H, W = 17, 23
    src = TC.randn(1, 2, H, W, seed=7) + 3.0             # no zeros in the source
    for ch in (0, 1):
        for sign in (1.0, -1.0):
            flow = np.zeros((1, 2, H, W), dtype=F32)
            flow[0, ch] = sign * far
            out = TC.warp2d(flow, src)
            assert (out == 0).all() and not np.signbit(out).any()
            assert (TC.memory_input(src[:, :1], src[:, 1:], flow)[:, 5] == 0).all()
            assert (TC.warp_labels2d(flow[None], np.full((1, H, W), 2, dtype=np.uint8), 4) == 0).all()
    flow3 = np.zeros((1, 3, 3, H, W), dtype=F32)
    flow3[0, 1] = far
    assert (TC.warp3d(flow3, TC.randn(1, 1, 3, H, W, seed=8) + 3.0) == 0).all()


def test_the_fin_guard_and_the_clamp():
    y = np.array([0.5, 1e6, 9.9e8, 1.1e9, 3e38, TC.NAN, TC.INF, -TC.INF, -1e6, -3e38], dtype=F32)
    t = TC.make_taps(y, np.full_like(y, 2.25), 17, 24)
    assert t["y0"].tolist() == [0, 18, 18, 18, 18, -2, 18, -2, -2, -2]                   # floor clamped to [-2, H + 1]; NaN -> -2
    assert t["v00"].tolist() == [True] + [False] * 9 and t["v10"].tolist() == [True] + [False] * 9
    assert np.isnan(t["w00"][5:8]).all() and np.isfinite(t["w00"][[0, 1, 2, 3, 4, 8, 9]]).all()
    t = TC.make_taps(np.array([-1.0, -0.25, 16.0, 16.5, 17.0], dtype=F32), np.array([-0.5, 23.0, 23.5, 3.0, 3.0], dtype=F32), 17, 24)
    # (y0, x0) = (-1, -1), (-1, 23), (16, 23), (16, 3), (17, 3) in a 17 x 24 image
    assert t["v00"].tolist() == [False, False, True, True, False] and t["v01"].tolist() == [False, False, False, True, False]
    assert t["v10"].tolist() == [False, True, False, False, False] and t["v11"].tolist() == [True, False, False, False, False]


# ===================================================================================================== resolving power
def test_corner_weights_show_on_invalid_taps_only():
    """module docstring: where (yf + 1) - y and 1 - (y - yf) differ, the weight belongs to a row outside the image"""
    y = np.array([-1e-3, -0.1, -2.0 ** -30, 2.0 ** 24, 3e7, 1e6, 5.3, 0.001, -5.3, 16.999], dtype=F32)
    a, b = TC.make_taps(y, y, 1 << 20, 1 << 20), TC.make_taps(y, y, 1 << 20, 1 << 20, variant="corner_weights")
    differs = a["w00"] != b["w00"]
    assert differs[:5].all() and not differs[5:].any()
    assert not (a["v00"] | a["v01"] | a["v10"])[differs].any()                            # every tap that carries ey or ex is invalid there
    assert np.array_equal(a["w11"], b["w11"])                                             # wy wx: the same in both
    rng = np.random.default_rng(9)
    y, x = (rng.uniform(-3, 40, 200000).astype(F32), rng.uniform(-3, 40, 200000).astype(F32))
    a, b = TC.make_taps(y, x, 17, 24), TC.make_taps(y, x, 17, 24, variant="corner_weights")
    for w, v in (("w00", "v00"), ("w01", "v01"), ("w10", "v10"), ("w11", "v11")):
        assert (a[w] != b[w]).sum() > 0 or w == "w11"
        assert np.array_equal(a[w][a[v]], b[w][a[v]])
    for name in TC.WARP_ROWS:
        flows, src = TC.warp_row_inputs(name)
        for f in flows.values():
            assert differing(TC.warp2d(f, src), TC.warp2d(f, src, variant="corner_weights")) == 0


@pytest.mark.parametrize("variant", ["contracted", "pairwise"])
@pytest.mark.parametrize("name", list(TC.WARP_ROWS))
def test_warp_rows_resolve(name, variant):
    flows, src = TC.warp_row_inputs(name)
    for fname, f in flows.items():
        assert differing(TC.warp2d(f, src), TC.warp2d(f, src, variant=variant)) > 0, (name, fname, variant)


@pytest.mark.parametrize("variant", ["contracted", "pairwise"])
@pytest.mark.parametrize("name", [n for n, r in TC.VECINT_ROWS.items() if r[3] > 0])
def test_vecint_rows_resolve(name, variant):
    """nsteps 0 is the scaling alone: no tap sum to vary (the GPU row asserts the exact scaling)"""
    vec, nsteps = TC.vecint_row_inputs(name)
    assert differing(TC.vecint2d(vec, nsteps), TC.vecint2d(vec, nsteps, variant=variant)) > 0


def test_vecint_nan_spreads_by_taps():
    """one NaN pixel, nsteps 2: after a step a pixel is NaN when its own value was, or when it is non-finite in position -- a NaN tap value
    times any weight (0 included) -- so the set grows by the pixels that sample the NaN; it stays a small neighbourhood"""
    vec, nsteps = TC.vecint_row_inputs("3x20x32 nsteps 2, one NaN")
    out = TC.vecint2d(vec, nsteps)
    nan = np.isnan(out)
    assert nan[1, 0, 9, 14] and 1 <= nan.sum() <= 64 and not nan[[0, 2]].any()
    ii, jj = np.nonzero(nan[1].any(0))
    assert np.abs(ii - 9).max() <= 8 and np.abs(jj - 14).max() <= 8


@pytest.mark.parametrize("name", list(TC.LABEL_ROWS))
def test_label_rows_resolve(name):
    K = TC.LABEL_ROWS[name][2]
    flow, random, checker = TC.label_row_inputs(name)
    for tag, lab in (("random", random), ("checkerboard", checker)):
        base, tie = TC.warp_labels2d(flow, lab, K), TC.warp_labels2d(flow, lab, K, variant="last_tie")
        assert (base != tie).sum() > 0, (name, tag)
        assert base.max() <= K - 1
    base, tie = TC.warp_labels2d(flow, checker, K), TC.warp_labels2d(flow, checker, K, variant="last_tie")
    H, W = checker.shape[1:]
    # frame 1, half-integer flows on the checkerboard: where all four taps stay inside (|flow| <= 4.5, five pixels from the border) the
    # two classes meet at 0.5 each, up to the ulp by which (i + f) misses the half pixel after the normalisation (15 and W - 1 are no
    # powers of two): most of these pixels are exact ties, which `>` and `>=` break differently, and the rest are decided by one rounding
    inner = (slice(None), slice(5, H - 5), slice(5, W - 5))
    mild = (np.abs(flow[1]) <= 4.5).all(1)[inner]
    assert mild.sum() > 50 and (base[1][inner][mild] != tie[1][inner][mild]).mean() > 0.5


@pytest.mark.parametrize("variant", ["contracted", "pairwise"])
@pytest.mark.parametrize("name", list(TC.MEMORY_ROWS))
def test_memory_rows_resolve(name, variant):
    x0, xt, flows = TC.memory_row_inputs(name)
    for fname, cum in flows.items():
        a, b = TC.memory_input(x0, xt, cum), TC.memory_input(x0, xt, cum, variant=variant)
        assert differing(a[:, 5], b[:, 5]) > 0, (name, fname)
        assert np.array_equal(a[:, :4], b[:, :4], equal_nan=True)


@pytest.mark.parametrize("variant", ["contracted", "pairwise"])
def test_sample_points_and_lookup_rows_resolve(variant):
    field, pts = TC.sample_points_inputs()
    assert differing(TC.sample_points(field, pts), TC.sample_points(field, pts, variant=variant)) > 0
    for name, r in TC.LOOKUP_ROWS.items():
        f1, f2, coords = TC.lookup_row_inputs(name)
        pyr = cpu_pyramid(f1, f2, r[4])
        assert differing(TC.corr_lookup(pyr, coords, r[5]), TC.corr_lookup(pyr, coords, r[5], variant=variant)) > 0, name


def test_warp3d_rows_resolve():
    flows, src = TC.warp3d_inputs()
    for fname, f in flows.items():
        assert differing(TC.warp3d(f, src), TC.warp3d(f, src, variant="contracted")) > 0, fname


# ===================================================================================================== fp64 sanity
@pytest.mark.parametrize("name", ["v4 2x3x17x24", "one-pixel 2x5x17x23"])
def test_tap_sum_against_fp64(name):
    """three additions and four products round, one spare: |chain - fp64| <= 8 x 2^-24 x sum |tap| w, on the chain's own taps and weights"""
    flows, src = TC.warp_row_inputs(name)
    for fname, f in flows.items():
        out, d = TC.warp2d(f, src, detail=True)
        taps = [d[k].astype(F64) for k in "abcd"]
        ws = [d[k].astype(F64)[:, None, :] for k in ("w00", "w01", "w10", "w11")]
        with np.errstate(invalid="ignore"):
            exact = sum(t * w for t, w in zip(taps, ws))
            mag = sum(np.abs(t) * w for t, w in zip(taps, ws))
        got = out.reshape(exact.shape).astype(F64)
        fin = np.isfinite(exact)
        assert np.array_equal(np.isnan(got), ~fin), fname
        assert (np.abs(got - exact)[fin] <= 8 * 2.0 ** -24 * mag[fin]).all(), (name, fname, float((np.abs(got - exact)[fin] / np.maximum(mag[fin], 1e-300)).max()))
        assert (mag[fin] > 0).sum() > got.size // 3
