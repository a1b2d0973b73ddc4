"""cf_batch_norm_coef and cf_coef_apply (csrc/norm_coef.hip) against an fp64 evaluation of the same formula.

Bars (no new number; u = 2^-24, tests/_norm_refs.py's derivations):
  table    mean and shift are copies: bitwise.  scale = gamma / sqrt(var + eps) is formed in fp64 and rounded once: 2^-23 |scale|, twice
           that rounding.
  apply    the affine part is gn_apply's chain (x - mean, * scale, + shift in fp32 on an fp32 table): _norm_refs' apply bar, 2^-21 M with
           M = (|x| + |mean|) |scale| + |shift|; behind an activation 1.13 * 2^-21 M + E_act + 2^-23 |ref| (1.13: the largest slope, GELU's;
           Mish's is 1.09).  coef == NULL has M = 0: 'none' and 'relu' are then exact, 'lrelu' one rounded product.
  E_act    none, relu, lrelu: 0.  gelu, tanh, sigmoid, mish: the error of the SAME fp32 formula evaluated by torch on the CPU against fp64
           (gelu: _norm_refs.gelu_as_f32, common.h's polynomial; mish: v > 20 ? v : v n / (n + 2), n = e (e + 2), e = exp(v)), times 2 for
           another order of roundings -- the worst over a dense sweep of [-31, 31], taken per binade of |v| so that the large
           arguments (half an ulp of 30 is 1e-6) do not set the bar of the small ones.
Cases: every activation, LeakyReLU slopes 0 / 0.01 / 0.2, with and without a table, in and out of place, the shapes (1,1,1), (2,3,35),
(1,5,4), (3,7,1023), rows misaligned by one float (16-byte body behind a scalar head) and x / out misaligned differently (the scalar
kernel), 18 000 rows of 5 values (a second grid trip: one trip covers 16 384 wave units on 256 CUs) and an NCDHW tensor.  Values of both
signs with |v| up to 30 (Mish's large-argument branch, GELU's saturated tails).  Measured ratios: profiles/variant_table.md."""
import math

import numpy as np
import pytest
import torch

import _norm_refs as R

pytestmark = pytest.mark.gpu

U = R.U
EPS = R.EPS
ACTS = [("none", 0.0), ("relu", 0.0), ("lrelu", 0.0), ("lrelu", 0.01), ("lrelu", 0.2), ("gelu", 0.0), ("tanh", 0.0), ("sigmoid", 0.0), ("mish", 0.0)]
SHAPES = [(1, 1, 1), (2, 3, 35), (1, 5, 4), (3, 7, 1023)]


def act64(v, act, slope):
    if act == "lrelu":
        return torch.where(v > 0, v, float(np.float32(slope)) * v)
    if act == "mish":
        return v * torch.tanh(torch.nn.functional.softplus(v, threshold=1e9))
    return R.act64(v, act)


def act_f32(v, act):
    """the kernel's formula in fp32 on the CPU (transcendental activations only)"""
    if act == "mish":
        e = torch.exp(v)
        n = e * (e + 2.0)
        return torch.where(v > 20.0, v, v * (n / (n + 2.0)))
    return R.act_f32(v, act)


_E = {}


def e_act(v, act):
    """2 x the fp32 formula's own error against fp64, the worst per binade of |v| over the sweep (binades clamped to [2^-8, 2^4])"""
    if act in ("none", "relu", "lrelu"):
        return torch.zeros_like(v)
    if act not in _E:
        s = torch.cat([torch.linspace(-31.0, 31.0, 2 ** 18 + 1, dtype=torch.float64), torch.logspace(-8.0, 1.49, 4001, dtype=torch.float64),
                       -torch.logspace(-8.0, 1.49, 4001, dtype=torch.float64)]).float()
        err = (act_f32(s, act).double() - act64(s.double(), act, 0.0)).abs()
        _E[act] = torch.zeros(13, dtype=torch.float64).scatter_reduce(0, _binade(s.double()), err, "amax")
    return 2.0 * _E[act][_binade(v)]


def _binade(v):
    return (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -8))).clamp(-8, 4) + 8).long()


def make_case(B, C, HW, seed, table=True):
    g = torch.Generator().manual_seed(seed)
    x = (10.0 * torch.randn(B, C, HW, generator=g)).clamp(-30.0, 30.0)
    flat = x.view(-1)
    for i, val in enumerate((30.0, -30.0, 25.0, -25.0, 20.5, 0.0)[:flat.numel()]):
        flat[(i * 7919) % flat.numel()] = val
    if not table:
        return x, None
    coef = torch.stack([0.3 * torch.randn(B, C, generator=g), 1.0 + 0.05 * torch.randn(B, C, generator=g), 0.2 * torch.randn(B, C, generator=g)], 1)
    return x, coef.contiguous()


def refs(x, coef, act, slope):
    """(ref, bar) in fp64 of act((x - mean) * scale + shift); x [B, C, HW] fp32, coef [B, 3, C] fp32 or None"""
    xd = x.double()
    if coef is None:
        v, M = xd, torch.zeros_like(xd)
    else:
        m, sc, sh = (coef[:, i].double()[..., None] for i in range(3))
        v = (xd - m) * sc + sh
        M = (xd.abs() + m.abs()) * sc.abs() + sh.abs()
    ref = act64(v, act, slope)
    if act == "none":
        return ref, 2.0 ** -21 * M
    return ref, 1.13 * 2.0 ** -21 * M + e_act(v, act) + 2.0 ** -23 * ref.abs()


def run(dev, x, coef, act, slope, inplace, x_off=0, out_off=None):
    """the call on device copies; x_off / out_off: the tensors start that many floats into a larger buffer (out_off None: in place or fresh)"""
    from cineflow import ops
    buf = torch.full((x.numel() + 8,), float("nan"), device=dev)
    xd = buf[x_off:x_off + x.numel()].view(x.shape)
    xd.copy_(x)
    cd = None if coef is None else coef.to(dev)
    if inplace:
        out = ops.coef_apply(xd, cd, act, slope, out=xd)
    elif out_off is None:
        out = ops.coef_apply(xd, cd, act, slope)
    else:
        obuf = torch.full((x.numel() + 8,), float("nan"), device=dev)
        out = ops.coef_apply(xd, cd, act, slope, out=obuf[out_off:out_off + x.numel()].view(x.shape))
        assert bool(torch.isnan(obuf[:out_off]).all()) and bool(torch.isnan(obuf[out_off + x.numel():]).all()), "a write outside out"
    if not inplace:
        assert torch.equal(xd.cpu(), x), "x was written"
    assert bool(torch.isnan(buf[:x_off]).all()) and bool(torch.isnan(buf[x_off + x.numel():]).all()), "a write outside x"
    return out.cpu()


@pytest.mark.parametrize("act,slope", ACTS)
def test_coef_apply_every_shape_and_form(dev, act, slope):
    worst = {}
    for si, (B, C, HW) in enumerate(SHAPES):
        for table in (True, False):
            x, coef = make_case(B, C, HW, 100 + si, table)
            ref, bar = refs(x, coef, act, slope)
            forms = [("out-of-place", dict(inplace=False)), ("in-place", dict(inplace=True)), ("head+1", dict(inplace=True, x_off=1)),
                     ("x+1/out+0", dict(inplace=False, x_off=1, out_off=0)), ("x+3/out+3", dict(inplace=False, x_off=3, out_off=3))]
            for form, kw in forms:
                r = R.ratio(run(dev, x, coef, act, slope, **kw), ref, bar)
                key = "table" if table else "NULL"
                worst[key] = max(worst.get(key, 0.0), r)
                assert r <= 1.0, "%s slope %g %s %s %s: %.3f x its bar" % (act, slope, (B, C, HW), key, form, r)
    print("\n  coef_apply %-7s slope %-4g worst |out - ref| / bar: with a table %.4f, coef == NULL %.4f" % (act, slope, worst["table"], worst["NULL"]))


@pytest.mark.parametrize("act,slope", [("lrelu", 0.2), ("mish", 0.0)])
def test_coef_apply_second_grid_trip_and_ncdhw(dev, act, slope):
    from cineflow import ops
    x, coef = make_case(3, 6000, 5, 7)                      # 18 000 rows: more wave units than one grid's worth
    ref, bar = refs(x, coef, act, slope)
    r = R.ratio(run(dev, x, coef, act, slope, inplace=True), ref, bar)
    x5, coef5 = make_case(2, 3, 4 * 5 * 7, 8)
    ref5, bar5 = refs(x5, coef5, act, slope)
    got5 = ops.coef_apply(x5.view(2, 3, 4, 5, 7).to(dev), coef5.to(dev), act, slope)
    assert got5.shape == (2, 3, 4, 5, 7)
    r5 = R.ratio(got5.cpu().view(2, 3, -1), ref5, bar5)
    print("\n  coef_apply %-5s 18 000 rows x 5: %.4f   NCDHW [2,3,4,5,7]: %.4f" % (act, r, r5))
    assert r <= 1.0 and r5 <= 1.0


def test_coef_apply_reads_group_norm_coef(dev):
    """IN / GN under LeakyReLU(0.2) or Mish: the table comes from cf_group_norm_coef (its rows are held to fp64 by the norm tests'
    coef rows); the pass is held to the table as the device wrote it"""
    from cineflow import ops
    B, C, HW, G = 2, 8, 35, 4
    x = R.make_data("std", (B, C, HW), 31)
    gamma, beta = 1.0 + 0.1 * R.randn(C, seed=32), 0.1 * R.randn(C, seed=33)
    xd = x.to(dev)
    coef = ops.group_norm_coef(ops.group_norm_stats(xd, G), gamma.to(dev), beta.to(dev), G, B, C, HW)
    for act, slope in (("lrelu", 0.2), ("mish", 0.0)):
        ref, bar = refs(x, coef.cpu(), act, slope)
        r = R.ratio(ops.coef_apply(xd, coef, act, slope).cpu(), ref, bar)
        print("\n  group_norm_coef -> coef_apply %s: %.4f" % (act, r))
        assert r <= 1.0
    # ... and the table is GroupNorm's: the normalised map has the group statistics (0, 1) under gamma = 1, beta = 0
    one = ops.group_norm_coef(ops.group_norm_stats(xd, G), None, None, G, B, C, HW)
    y = ops.coef_apply(xd, one, None).cpu().double().view(B, G, -1)
    assert float(y.mean(-1).abs().max()) <= 1e-5 and float((y.var(-1, unbiased=False) - 1.0).abs().max()) <= 1e-4


@pytest.mark.parametrize("B,C,affine", [(1, 1, True), (2, 7, True), (3, 300, True), (2, 5, False)])
def test_batch_norm_coef(dev, B, C, affine):
    from cineflow import ops
    g = torch.Generator().manual_seed(40 + C)
    rm, rv = 0.5 * torch.randn(C, generator=g), (0.02 + torch.rand(C, generator=g) * 3.0)
    rv[0] = 0.0                                                                       # a dead channel: scale = gamma / sqrt(eps)
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)) if affine else (None, None)
    coef = ops.batch_norm_coef(rm.to(dev), rv.to(dev), None if gamma is None else gamma.to(dev), None if beta is None else beta.to(dev), B).cpu()
    assert coef.shape == (B, 3, C)
    scale = (torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()) / torch.sqrt(rv.double() + EPS)
    for b in range(B):
        assert torch.equal(coef[b, 0], rm) and torch.equal(coef[b, 2], torch.zeros(C) if beta is None else beta)
        r = R.ratio(coef[b, 1], scale, 2.0 ** -23 * scale.abs())
        assert r <= 1.0, r
    print("\n  batch_norm_coef B %d C %3d: scale within %.3f of 2^-23 |scale|" % (B, C, R.ratio(coef[0, 1], scale, 2.0 ** -23 * scale.abs())))


def test_host_refusals_need_no_launch(dev):
    from cineflow import ops
    from cineflow._lib import CineflowError
    assert ops.coef_apply_ok(2, 3, 35) and not ops.coef_apply_ok(2, 3, 2 ** 30 + 1) and not ops.coef_apply_ok(2 ** 20, 2 ** 11, 2 ** 10)
    x = torch.zeros(1, 2, 4, device=dev)
    with pytest.raises(CineflowError, match="slope"):
        ops.coef_apply(x, None, "lrelu", -0.5)
    with pytest.raises(KeyError):
        ops.coef_apply(x, None, "swish")
    assert math.isfinite(float(ops.coef_apply(x, None, "mish").sum()))
