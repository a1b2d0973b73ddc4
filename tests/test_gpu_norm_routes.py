"""The ten kernel instantiations of csrc/norm.hip behind cf_group_norm*, cf_layer_norm_cf, cf_group_norm_coef and cf_norm_head_1x1, each row
held to the fp64 reference and the derived bar of tests/_norm_refs.py (derivations in that module's docstring) and, for the GroupNorm
launchers, to the plan cf_group_norm_route returns -- the plan the launchers execute, so a row cannot pass on another kernel or geometry.

Every row writes into a buffer of sentinels (7.0, 64 floats on either side) that must come back untouched, its output NaN-filled before
the call; "view" rows read their input one float into a NaN-fenced buffer (_split_exact.device_input).  pytest -s prints one line per row
and form: the plan and the worst |out - ref| / bar; profiles/norm_route_table.md lists them beside the CPU emulation of
test_norm_refs_cpu.py, which also shows that every near-miss reference of a row lies beyond its bar.

  statistics   gn_stats_wave_kernel / gn_stats_block_kernel: the L = 4096 | 4100 line, a lone float4 in a last sweep, L < 64, slab counts
               that are no multiple of 4, the clamp of segs at 64, misaligned input, offset data (mean / std = 64) on both routes
  apply        gn_apply_small_kernel<0|1> / gn_apply_kernel<0|1> from host fp64 sums: every geometry line of the launcher, six forms each
               (plain, GELU with a residual on either side, LeakyReLU, a normalised residual on either side), in place, misaligned x or
               res alone, offset and small-variance data, constant slabs (bitwise beta)
  composed     cf_group_norm (statistics + apply) against fp64 GroupNorm of the input, and the production z-score call (groups 1, eps 0,
               no affine, in place) with an all-zero and a constant frame
  LayerNorm    layer_norm_cf_kernel: C = 256 | 257, C = 1, 8, 9, N = 1, a block with one valid token, in place on both paths
  gn_coef      gn_coef_kernel on one and two thread blocks, null affine, a constant slab
  head         norm_head_1x1_kernel<2|4|8>: one pixel group, a second block with one float4, the LDS maximum, slope 0, bias or none
  activations  act_apply through an identity normalisation over [-12, 12] (2^21 + 1 points), +-1e-30 .. 16 (logarithmic), zeros, the
               smallest normal, a denormal, +-65504, +-1e30, NaN and the infinities

Measured on the MI355X (profiles/norm_route_table.md has every row): worst |out - ref| / bar 0.36 over the apply rows, 0.33 composed, 0.37
LayerNorm, 0.15 head, 0.48 GELU sweep, 0.010 block statistics, < 1e-4 wave statistics; relative variance error at mean / std = 64: 1.9e-13 on
the wave route, 8.8e-6 on the block route (inside its bar: the block kernel is left as it is).  The z-score call returns NaN for every
element of an all-zero and of a constant frame on both routes (0 x inf).  gelu(-inf) is NaN.  One defect found: relu(NaN) was 0
(every other activation, and torch.relu, return NaN); the apply passes now keep it (norm_act in norm.hip), finite values, -0 and the
infinities bitwise as before.  act_apply, which the convolution epilogues share, is unchanged: there the extra instruction was measurable.

Where the rows differ from the list they were written from, and why: (2, 4, 2048, 2) is L = 4096, the wave kernel whatever the alignment, so
(2, 4, 4096, 2) "view" is added for the misaligned L = 8192; 64 x 64 frames are L = 4096, still the wave kernel, so 128 x 128 is added to
the z-score frames for the block kernel; -0 through the identity normalisation returns +0 (-0 + beta, beta = +0), the one input
excepted from "bitwise"; LeakyReLU's reference in the sweep is the exact product float32(0.01) v rounded once -- what an fp32 multiply
returns -- since no fp32 kernel can meet a bar of 0 against the unrounded fp64 product.

gn_apply_stem_kernel<1|6> is pinned bitwise to the stored-residual pass by test_gpu_stem_apply.py and is not repeated here."""
import numpy as np
import pytest
import torch

import _norm_refs as R
from _split_exact import device_input

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 7.0
PAD = 64
EPS32 = 1e-5                                   # the float argument; the kernels widen float32(1e-5) = R.EPS
_ids = lambda rows: [r.name for r in rows]


def fenced(dev, shape, init=None, dtype=torch.float32):
    """(buffer, out): out is a view `PAD` elements into a buffer of sentinels, NaN-filled (or holding init)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, device=dev, dtype=dtype)
    out = buf[PAD:PAD + n].view(shape)
    if init is None:
        out.fill_(NAN)
    else:
        out.copy_(init.to(dev))
    assert out.data_ptr() % 16 == 0 and out.is_contiguous()
    return buf, out


def fence_intact(buf, what):
    host = buf.cpu()
    assert bool((host[:PAD] == SENT).all()) and bool((host[-PAD:] == SENT).all()), "%s: the kernel wrote outside its output" % what


def dv(t, dev):
    return None if t is None else t.to(dev)


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.STATS_ROWS, ids=_ids(R.STATS_ROWS))
def test_statistics_rows(dev, row):
    from cineflow import ops
    from cineflow._lib import check, lib
    c = R.stats_case(row)
    xd = device_input(c["x"], dev, row.view)
    plan = ops.group_norm_route(xd, None, None, row.groups)
    assert tuple(plan[:3]) == row.plan, "%s: planned %s, the row is for %s" % (row.name, tuple(plan[:3]), row.plan)
    buf, ws = fenced(dev, (row.B, row.groups, 2), dtype=torch.float64)
    check(lib().cf_group_norm_stats(xd.data_ptr(), ws.data_ptr(), row.B, row.C, row.HW, row.groups, torch.cuda.current_stream().cuda_stream),
          "cf_group_norm_stats")
    got = ws.cpu()
    fence_intact(buf, row.name)
    worst = R.ratio(got, c["ref"], c["bar"])
    again = R.ratio(ops.group_norm_stats(xd, row.groups).cpu(), c["ref"], c["bar"])
    var = R.variance_of(c["ref"], c["L"])
    relvar = float(((R.variance_of(got, c["L"]) - var).abs() / var).max())
    print("\n  stats %-26s plan %-12s |ws - ref| / bar %.4f (wrapper %.4f)  relative variance error %.2e" % (
        row.name, tuple(plan[:3]), worst, again, relvar))
    assert worst <= 1.0 and again <= 1.0, "%s: %.3f, %.3f x its bar" % (row.name, worst, again)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
def run_apply(dev, row, inp, form, composed=False, eps=EPS32):
    """the route, then ops.group_norm_apply (or ops.group_norm) of one form into a fenced output -> (out on the CPU, plan)"""
    from cineflow import ops
    kw = R.form_kwargs(inp, form)
    xd = device_input(inp["x"], dev, row.view == "x")
    if row.inplace:
        buf, out = fenced(dev, xd.shape, init=inp["x"])
        xd = out
    else:
        buf, out = fenced(dev, xd.shape)
    resd = device_input(kw["res"], dev, row.view == "res") if "res" in kw else None
    plan = tuple(ops.group_norm_route(xd, out, resd, row.groups))
    assert plan == row.plan, "%s %s: planned %s, the row is for %s" % (row.name, form, plan, row.plan)
    args = dict(act=kw["act"], res=resd, res_mode=kw.get("res_mode"), out=out)
    if composed:
        assert "res_norm" not in kw
        ops.group_norm(xd, dv(kw["gamma"], dev), dv(kw["beta"], dev), row.groups, eps=eps, **args)
    else:
        rn = tuple(dv(t, dev) for t in kw["res_norm"]) if "res_norm" in kw else None
        ops.group_norm_apply(xd, dv(kw["gamma"], dev), dv(kw["beta"], dev), row.groups, inp["ws"].to(dev), eps=eps, res_norm=rn, **args)
    got = out.cpu()
    fence_intact(buf, "%s %s" % (row.name, form))
    return got, plan


@pytest.mark.parametrize("row", R.APPLY_ROWS, ids=_ids(R.APPLY_ROWS))
def test_apply_rows(dev, row):
    inp = R.apply_inputs(row)
    for form in R.forms_of(row):
        got, plan = run_apply(dev, row, inp, form)
        ref, bar = R.apply_refs(inp["x"], inp["ws"], groups=row.groups, **R.form_kwargs(inp, form))
        worst = R.ratio(got, ref, bar)
        print("\n  apply %-26s %-20s plan %-30s |out - ref| / bar %.4f" % (row.name, form, plan, worst))
        assert worst <= 1.0, "%s %s: %.3f x its bar (NaN: an element no block wrote, or a read outside an input)" % (row.name, form, worst)


@pytest.mark.parametrize("row", [r for r in R.APPLY_ROWS if r.name in ("small-vec-one-short-block", "large-vec-asegs1")], ids=lambda r: r.name)
def test_apply_constant_slabs_give_beta_bitwise(dev, row):
    inp = R.constant_slab_inputs(row)
    got, _ = run_apply(dev, row, inp, "plain")
    cpg = row.C // row.groups
    for slab in (0, 1):
        b, g = divmod(slab, row.groups)
        want = inp["beta"].float()[g * cpg:(g + 1) * cpg, None].expand(cpg, row.HW).contiguous()
        assert torch.equal(got[b, g * cpg:(g + 1) * cpg].contiguous().view(torch.int32), want.view(torch.int32)), (row.name, slab)
    ref, bar = R.apply_refs(inp["x"], inp["ws"], inp["gamma"], inp["beta"], row.groups)
    assert R.ratio(got, ref, bar) <= 1.0


COMPOSED = ("large-vec-asegs1", "large-vec-asegs2", "small-vec-one-short-block", "small-offset", "large-offset")


@pytest.mark.parametrize("name", COMPOSED + ("stats-offset-wave", "stats-offset-block"))
def test_composed_group_norm(dev, name):
    """cf_group_norm against fp64 GroupNorm of the input: the apply bar plus the statistics bar of the route taken, propagated"""
    if name.startswith("stats-"):
        s = [r for r in R.STATS_ROWS if r.name == name[6:]][0]
        plan = {"offset-wave": (0, 0, 4, 0, 1, 8, 4, 8), "offset-block": (1, 1, 16, 1, 1, 1, 32, 0)}[s.name]
        row = R.ApplyRow(name, s.B, s.C, s.HW, s.groups, "", False, "offset", plan, False)
        x = R.make_data("offset", (s.B, s.C, s.HW), seed=1000 + s.HW)
        p = R.randn(2, s.C, seed=1001)
        inp = dict(x=x, gamma=1.0 + 0.5 * p[0], beta=p[1], ws=R.host_ws(x, s.groups), res=R.make_data("std", x.shape, seed=1002))
    else:
        row = [r for r in R.APPLY_ROWS if r.name == name][0]
        inp = R.apply_inputs(row)
    for form in ("plain", "gelu+res-after"):
        got, plan = run_apply(dev, row, inp, form, composed=True)
        kw = R.form_kwargs(inp, form)
        ref, bar = R.apply_refs(inp["x"], inp["ws"], groups=row.groups, **kw)
        extra = R.propagate_stats_bar(inp["x"], inp["ws"], kw["gamma"], row.groups, R.EPS, block=plan[0] == 1)
        worst, alone = R.ratio(got, ref, bar + 1.13 * extra), R.ratio(got, ref, bar)
        print("\n  composed %-26s %-16s plan %-30s |out - ref| / bar %.4f (against the apply bar alone %.4f)" % (row.name, form, plan, worst, alone))
        assert worst <= 1.0, "%s %s: %.3f x its bar" % (row.name, form, worst)


@pytest.mark.parametrize("side, stats_plan", ((32, (0, 0, 2)), (64, (0, 0, 2)), (128, (1, 2, 10))))
def test_production_z_score_in_place(dev, side, stats_plan):
    """ops.group_norm(flat, None, None, 1, eps=0, out=flat) on [T, 1, H W] as inference.py and mtl.py call it: an all-zero frame and a
    constant frame come back uniform -- every element non-finite, or every element exactly 0 -- which is what Processor.discretize relies
    on; the other frames stay within the composed bar.  (64 x 64 is L = 4096: still the wave kernel; 128 x 128 takes the block kernel.)"""
    from cineflow import ops
    T, HW = 5, side * side
    x = R.make_data("zscore", (T, 1, HW), seed=1100 + side)
    x[1], x[3] = 0.0, 300.0
    buf, flat = fenced(dev, x.shape, init=x)
    plan = tuple(ops.group_norm_route(flat, flat, None, 1))
    assert plan[:3] == stats_plan, plan
    ops.group_norm(flat, None, None, 1, eps=0.0, out=flat)
    got = flat.cpu()
    fence_intact(buf, "z-score")
    outcome = {}
    for t, what in ((1, "zero"), (3, "constant")):
        nonfinite, zero = bool((~torch.isfinite(got[t])).all()), bool((got[t] == 0).all())
        assert nonfinite or zero, "%s frame: neither uniformly non-finite nor uniformly 0" % what
        outcome[what] = "non-finite" if nonfinite else "0"
    keep = [0, 2, 4]
    xs, ws = x[keep], R.host_ws(x[keep], 1)
    ref, bar = R.apply_refs(xs, ws, None, None, 1, eps=0.0)
    bar = bar + R.propagate_stats_bar(xs, ws, None, 1, 0.0, block=plan[0] == 1)
    worst = R.ratio(got[keep], ref, bar)
    print("\n  z-score %3d x %-3d plan %-30s zero frame -> %s, constant frame -> %s; other frames |out - ref| / bar %.4f" % (
        side, side, plan, outcome["zero"], outcome["constant"], worst))
    assert worst <= 1.0


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.LN_ROWS, ids=_ids(R.LN_ROWS))
def test_layer_norm_rows(dev, row):
    from cineflow import ops
    inp = R.ln_inputs(row)
    xd = device_input(inp["x"], dev, row.view)
    buf, out = fenced(dev, xd.shape, init=inp["x"] if row.inplace else None)
    if row.inplace:
        xd = out
    ops.layer_norm_cf(xd, inp["gamma"].to(dev), inp["beta"].to(dev), eps=EPS32, out=out)
    got = out.cpu()
    fence_intact(buf, row.name)
    ref, bar = R.ln_refs(**inp)
    worst = R.ratio(got, ref, bar)
    print("\n  ln %-26s |out - ref| / bar %.4f" % (row.name, worst))
    assert worst <= 1.0, "%s: %.3f x its bar" % (row.name, worst)
    if row.C == 1:
        want = inp["beta"].float().view(1, 1, 1).expand(row.B, 1, row.N).contiguous()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- gn_coef ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.COEF_ROWS, ids=_ids(R.COEF_ROWS))
def test_coef_rows(dev, row):
    from cineflow._lib import check, lib
    inp = R.coef_inputs(row)
    buf, coef = fenced(dev, (row.B, 3, row.C))
    ptr = lambda t: None if t is None else t.data_ptr()
    g, b, ws = dv(inp["gamma"], dev), dv(inp["beta"], dev), inp["ws"].to(dev)
    check(lib().cf_group_norm_coef(ws.data_ptr(), ptr(g), ptr(b), row.B, row.C, row.HW, row.groups, EPS32, coef.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "cf_group_norm_coef")
    got = coef.cpu()
    fence_intact(buf, row.name)
    rm, rs, same = R.coef_ratios(got, *R.coef_refs(row, inp))
    print("\n  coef %-24s blocks %d  mean / (u |mean|) %.3f  scale / (2^-22 |scale|) %.3f  shift bitwise %s" % (
        row.name, (row.B * row.C + 255) // 256, rm, rs, same))
    assert rm <= 1.0 and rs <= 1.0 and same


# ---- norm_head_1x1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.HEAD_ROWS, ids=_ids(R.HEAD_ROWS))
def test_head_rows(dev, row):
    from cineflow._lib import check, lib
    inp = R.head_inputs(row)
    buf, out = fenced(dev, (row.B, row.K, row.HW))
    x, coef, w, bias = (dv(inp[k], dev) for k in ("x", "coef", "w", "bias"))
    check(lib().cf_norm_head_1x1(x.data_ptr(), coef.data_ptr(), row.slope, w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(),
                                 row.B, row.C, row.HW, row.K, torch.cuda.current_stream().cuda_stream), "cf_norm_head_1x1")
    got = out.cpu()
    fence_intact(buf, row.name)
    ref, bar = R.head_refs(slope=row.slope, **inp)
    worst = R.ratio(got, ref, bar)
    print("\n  head %-28s LDS %5d bytes  |out - ref| / bar %.4f" % (row.name, 4 * (3 + row.K) * row.C, worst))
    assert worst <= 1.0, "%s: %.3f x its bar" % (row.name, worst)


# ---- activations -----------------------------------------------------------------------------------------------------------------------
def identity_apply(dev, v, act):
    """act(v) through group_norm_apply with a workspace that makes the normalisation the identity: mean 0, var + eps = 1, no affine"""
    from cineflow import ops
    n = v.numel()
    ws = torch.tensor([0.0, n * (1.0 - R.EPS)], dtype=torch.float64, device=dev)
    buf, out = fenced(dev, (1, 1, n))
    ops.group_norm_apply(v.view(1, 1, n).to(dev), None, None, 1, ws, eps=EPS32, act=act, out=out)
    got = out.cpu().view(-1)
    fence_intact(buf, "sweep %s" % act)
    return got


@pytest.mark.parametrize("part", ("dense", "tails"))
def test_activation_sweep(dev, part):
    v = R.sweep_inputs()[0 if part == "dense" else 1]
    same = identity_apply(dev, v, "none")
    neg0 = (v == 0) & torch.signbit(v)                                  # -0 + (beta = +0) is +0: the one input that does not come back bitwise
    assert torch.equal(same[~neg0].view(torch.int32), v[~neg0].view(torch.int32)) and bool((same[neg0] == 0).all())
    for act in R.ACTS[1:]:
        got = identity_apply(dev, v, act)
        ref, bar = R.sweep_refs(v, act)
        worst = R.ratio(got, ref, bar)
        at = float(v[int(((got.double() - ref).abs() / bar.clamp_min(1e-300)).nan_to_num(posinf=1e300).argmax())])
        print("\n  sweep %-6s %-8s worst |out - ref| / bar %.4f (at v = %.6g)" % (part, act, worst, at))
        assert worst <= 1.0, "%s: %.3f x its bar at v = %g" % (act, worst, at)


def test_activation_specials(dev):
    v = torch.tensor([NAN, float("inf"), float("-inf"), -1e30], dtype=torch.float32)
    got = {act: identity_apply(dev, v, act) for act in R.ACTS}
    for act in R.ACTS:
        assert bool(torch.isnan(got[act][0])), "%s(NaN) = %g" % (act, float(got[act][0]))
    for act in ("none", "gelu", "relu", "lrelu"):
        assert float(got[act][1]) == float("inf"), act
    assert float(got["gelu"][3]) == 0.0
    assert float(got["tanh"][1]) == 1.0 and float(got["tanh"][2]) == -1.0 and float(got["sigmoid"][1]) == 1.0 and float(got["sigmoid"][2]) == 0.0
    assert float(got["relu"][2]) == 0.0 and float(got["lrelu"][2]) == float("-inf")
    print("\n  specials: gelu(-inf) = %g (recorded, not asserted)" % float(got["gelu"][2]))
