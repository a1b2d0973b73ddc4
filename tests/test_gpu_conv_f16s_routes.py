"""Every instantiation of conv_f16s_kernel (csrc/conv_f16s.hip), in both product modes, against a split-exact fp64 reference.

f16s_plan picks one of the 30 template shapes <KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL> of its table (CF_F16S_SHAPES), each built with
TERMS = 3 (hi/lo split) and TERMS = 1 (hi x hi, ops.conv_terms(1)).  One row per shape (tests/_conv_f16s_rows.py), run under both modes:
60 instantiations.  Each row names its tuple and its images per workgroup and, in a comment, the condition that sends the layer there.
The routing is asserted: the launcher executes the plan that cf_conv2d_f16s_route exports, and every row asks it with the tensors it then
launches on, per product mode (test_abi_and_host.py asks the same of every row without a GPU).  A rocprofv3 kernel trace read by
tools/kernel_coverage.py is a cross-check on the device, not the evidence.

Reference.  The kernel multiplies exactly these fp16 operands:
    s, wh, wl        as pack_conv_weight_f16s makes them: ws = 2^s w (exact), wh = fp16(ws), wl = fp16(ws - wh)
    xh, xl           xh = fp16(x), xl = fp16(x - xh)     (x - xh is exact in fp32)
    y3 = 2^-s (conv(xh, wl) + conv(xl, wh) + conv(xh, wh)) + b          (TERMS = 3)
    y1 = 2^-s conv(xh, wh) + b                                          (TERMS = 1)
evaluated in float64 (conv_transpose2d on the same split operands for the transposed convolution).  A product of two fp16 values is exact
in fp32 and the 2^-s scaling is exact, so the kernel differs from y3 / y1 only by the rounding of its fp32 accumulation.

Bar.  Let A = 2^-s conv(|xh| + |xl|, |wh| + |wl|) + |b| (per output element; it bounds every partial sum and the biased result).  The
accumulator sees n = nchunk * taps * CK / 16 MFMAs per term; each adds 16 exact products and rounds once to fp32 (unit roundoff
u = 2^-24), and the epilogue's alpha * acc + b rounds once more.  The deterministic bound is |err| <= (n + 1) u A; rounding errors of
successive steps are independent and of either sign, so the error grows like sqrt(n) u A in practice.  The bar 2^-18 A = 64 u A holds
for n <= 63 with certainty and, as a random walk, up to n ~ 4000 (the rows here have n <= 30 per term, 90 with the lo terms).  It resolves what a
kernel bug looks like: the lo terms are ~2^-11 A (the one-term output fails the three-term bar, asserted per row), and one dropped
input channel, tap or chunk moves the output by ~A / sqrt(taps * C) >> 2^-18 A (a reference with the last input channel zeroed fails
the bar, asserted per row).  The worst measured ratio to the bar is printed per row (pytest -s).

The contract the rest of the suite keeps stands next to it: TERMS = 3 against the fp64 convolution of the true operands at 1e-5
absolute; TERMS = 1 against the same at 3 * 2^-11 A (fp16 rounding of both operands is <= 2^-11 relative each, plus fp32 accumulation).

Epilogue.  act(alpha * acc + b) + res into channels [2, 2 + Cout) of a wider tensor: checked against fp64 act(alpha * (y - b) + b) + res
with y the same launch's plain output (same accumulator, so only the epilogue's own fp32 rounding and the activation's polynomial
approximation remain: 2e-6 (1 + |pre| + |res|)), all five activations on every row (every staging form x mode); the sentinel channels
must stay untouched.  GroupNorm statistics (fused in the epilogue where every workgroup holds one sample, else the statistics pass) are
checked against fp64 sums of the stored output at the suite's 2e-6.

PRE rows normalise the input in fp32 while staging (lrelu / GELU of (x - mean) * scale + shift), so the split-exact reference does not
apply.  TERMS = 3 is compared with fp64 at the suite's 3e-5.  TERMS = 1 is compared with the two-pass route in the same mode
(group_norm_apply, then conv2d_f16s): both round fp32 activations that agree to a few fp32 ulps to fp16, so an operand's hi differs
between the routes by one fp16 ulp (2^-11 relative) only where an fp16 rounding boundary falls between them, for ~2^-12 of the operands;
the two routes also accumulate in different orders (2 x 2^-18 A).  A flip moves one product by 2^-11 of itself, and a product is a small
fraction of A (>= 216 products per output here): an output that collects a few flips on its largest products moves by ~2^-15 A.  The
bar is 2^-13 A (A of the two-pass operands), a quarter of the 2^-11 A that separates the one-term mode from the true operands; the
measured ratio is printed.

NARROW_ROWS run shapes of the table again on maps one to three columns wide and taller than one tile's staging budget, where f16s_plan
gives the tile fewer rows: the part-filled tiles and the second tile along y are what those rows add.

Large rows compare only a few samples against the CPU reference: the first, the last and the two on either side of the first
multi-image workgroup boundary.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from _conv_f16s_rows import CONVT_ROWS, NARROW_ROWS, PAD, PRE_ROWS, ROWS, row_id
from _split_exact import (ACTS, SPLIT_BAR, TORCH_ACT, check_stats, device_input, randn, ratio, samples_of, split_reference, split_w,
                          split_x)

pytestmark = pytest.mark.gpu

ONE_TERM_BAR = 3 * 2.0 ** -11
PRE_ONE_TERM_BAR = 2.0 ** -13


@pytest.mark.parametrize("row", ROWS + NARROW_ROWS, ids=row_id)
def test_conv_f16s_route(dev, row):
    from cineflow import ops
    B, C, H, W, Cout, (kh, kw), stride = row.B, row.C, row.H, row.W, row.Cout, row.k, row.stride
    pad = PAD[row.k]
    seed = sum(row.tup) * 7 + B
    x = randn(B, C, H, W, seed=seed)
    w = randn(Cout, C, kh, kw, seed=seed + 1) / math.sqrt(C * kh * kw)
    b = randn(Cout, seed=seed + 2)
    groups = 8 if Cout % 8 == 0 else Cout
    sm = samples_of(B, row.nimg)
    xd, bd = device_input(x, dev, row.view), b.to(dev)
    wpk, s = ops.pack_conv_weight_f16s(w.to(dev))
    Ho, Wo = (H + 2 * pad[0] - kh) // stride + 1, (W + 2 * pad[1] - kw) // stride + 1
    res = randn(B, Cout, Ho, Wo, seed=seed + 3)
    resd = res.to(dev)
    ref = split_reference(x[sm], w, b, s, lambda a, m: F.conv2d(a, m, stride=stride, padding=pad))
    bar = SPLIT_BAR * ref["A"]
    outs, worst = {}, {}
    for terms in (3, 1):
        with ops.conv_terms(terms):
            plan = ops.conv2d_f16s_route(xd, Cout, kh, kw, stride, pad, stats_groups=groups)
            assert (plan.route, plan.tup, plan.terms, plan.nimg, plan.fused, plan.part) == (1, row.tup, terms, row.nimg, row.nimg == 1, B), plan
            out, st = ops.conv2d_f16s(xd, wpk, s, bd, Cout, kh, kw, stride, pad, stats_groups=groups)
            epi = {}
            for act in ACTS:
                big = torch.full((B, Cout + 5, Ho, Wo), 7.0, device=dev)
                ops.conv2d_f16s(xd, wpk, s, bd, Cout, kh, kw, stride, pad, act=act, res=resd, out=big, out_coff=2, alpha=0.75)
                assert bool((big[:, :2] == 7.0).all()) and bool((big[:, 2 + Cout:] == 7.0).all()), (act, "sentinel channels written")
                epi[act] = big[sm, 2:2 + Cout].cpu().double()
        torch.cuda.synchronize()
        o = out[sm].cpu().double()
        outs[terms] = o
        want = ref["y%d" % terms]
        worst[terms] = ratio(o, want, bar)
        assert worst[terms] <= 1.0, ("split-exact", terms, worst[terms])
        if terms == 3:
            d = float((o - ref["true"]).abs().max())
            assert d <= 1e-5, ("fp64 contract", d)
        else:
            r1 = ratio(o, ref["true"], ref["A"])
            assert r1 <= ONE_TERM_BAR, ("one-term vs fp64", r1)
        assert ratio(o, want - ref["d%d" % terms], bar) > 1.0, "a dropped last input channel would pass the bar"
        check_stats(out[sm].cpu(), st, B, groups, sm)
        pre = 0.75 * (o - b.double().view(1, -1, 1, 1)) + b.double().view(1, -1, 1, 1)
        rs = res[sm].double()
        for act in ACTS:
            e = TORCH_ACT[act](pre) + rs
            err = float(((epi[act] - e).abs() / (1.0 + pre.abs() + rs.abs())).max())
            assert err <= 2e-6, (terms, act, err)
    one_vs_three = ratio(outs[1], ref["y3"], bar)
    assert one_vs_three > 1.0, "the three-term bar does not resolve the lo terms"
    print("\n%s worst |out - ref| / (2^-18 A): TERMS=3 %.4f  TERMS=1 %.4f  (one-term output vs the three-term bar: %.0f)"
          % (row_id(row), worst[3], worst[1], one_vs_three))


@pytest.mark.parametrize("row", PRE_ROWS, ids=row_id)
def test_conv_f16s_prenorm_route(dev, row):
    from cineflow import ops
    B, C, H, W, Cout = row.B, row.C, row.H, row.W, row.Cout
    seed = sum(row.tup) * 11 + B
    x = randn(B, C, H, W, seed=seed) * 1.7 + 0.4
    g, bt = randn(C, seed=seed + 1), randn(C, seed=seed + 2)
    w = randn(Cout, C, 3, 3, seed=seed + 3) / math.sqrt(C * 9)
    b = randn(Cout, seed=seed + 4)
    sm = samples_of(B, 1)
    xd, gd, btd, bd = x.to(dev), g.to(dev), bt.to(dev), b.to(dev)
    assert ops.prenorm_ok(xd, Cout)
    wpk, s = ops.pack_conv_weight_f16s(w.to(dev))
    wh, wl = split_w(w, s)
    conv = lambda a, m: F.conv2d(a, m, padding=1)
    for groups, slope, act in ((8, -1.0, "gelu"), (C, 0.01, "lrelu")):
        xs = x.double().view(B, groups, -1)
        ws = torch.stack([xs.sum(-1), (xs ** 2).sum(-1)], -1).reshape(-1).to(dev)
        coef = ops.group_norm_coef(ws, gd, btd, groups, B, C, H * W)
        a64 = TORCH_ACT[act](F.group_norm(x[sm].double(), groups, g.double(), bt.double(), eps=1e-5))
        want = conv(a64, w.double()) + b.double().view(1, -1, 1, 1)
        for terms in (3, 1):
            with ops.conv_terms(terms):
                plan = ops.conv2d_f16s_route(xd, Cout, 3, 3, 1, (1, 1), prenorm=True, stats_groups=Cout)
                assert (plan.route, plan.tup, plan.terms, plan.nimg, plan.fused, plan.part) == (1, row.tup, terms, 1, True, B), plan
                out, st = ops.conv2d_f16s_prenorm(xd, coef, slope, wpk, s, bd, Cout, stats_groups=Cout)
                applied = ops.group_norm_apply(xd, gd, btd, groups, ws, act=act, out=torch.empty_like(xd))
                two = ops.conv2d_f16s(applied, wpk, s, bd, Cout, 3, 3, 1, (1, 1))
            o = out[sm].cpu().double()
            check_stats(out[sm].cpu(), st, B, Cout, sm)
            if terms == 3:
                d = float((o - want).abs().max())
                assert d <= 3e-5, (act, d)
                assert float((o - two[sm].cpu().double()).abs().max()) <= 2e-5
                print("\n%s %s TERMS=3 max|out - fp64| = %.2e (bar 3e-5)" % (row_id(row), act, d), end="")
            else:
                ah, al = split_x(applied[sm].cpu())
                A = 2.0 ** -s * conv(ah.abs() + al.abs(), wh.abs() + wl.abs()) + b.double().abs().view(1, -1, 1, 1)
                r = ratio(o, two[sm].cpu().double(), PRE_ONE_TERM_BAR * A)
                assert r <= 1.0, (act, r)
                assert ratio(o, want, A) <= ONE_TERM_BAR
                print("  TERMS=1 vs two-pass route: %.4f of the 2^-13 A bar" % r, end="")


@pytest.mark.parametrize("row", CONVT_ROWS, ids=row_id)
def test_conv_transpose_f16s_route(dev, row):
    from cineflow import ops
    B, Cin, H, W, Cout = row.B, row.Cin, row.H, row.W, row.Cout
    seed = sum(row.tup) * 13 + B
    x = randn(B, Cin, H, W, seed=seed)
    w = randn(Cin, Cout, 2, 2, seed=seed + 1) / math.sqrt(Cin)
    b = randn(Cout, seed=seed + 2)
    groups = 4
    sm = samples_of(B, row.nimg)
    wg = w.permute(1, 2, 3, 0).reshape(Cout * 4, Cin, 1, 1)         # GEMM rows (co, dy, dx)
    wpk, s = ops.pack_conv_weight_f16s(wg.to(dev))
    xd, bd = x.to(dev), b.to(dev)

    def convt(a, m):          # m in GEMM layout [4 Cout, Cin, 1, 1] (or one input channel of it)
        return F.conv_transpose2d(a, m.reshape(Cout, 2, 2, -1).permute(3, 0, 1, 2), stride=2)

    ref = split_reference(x[sm], wg, b, s, convt)
    bar = SPLIT_BAR * ref["A"]
    outs, worst = {}, {}
    for terms in (3, 1):
        with ops.conv_terms(terms):
            for g in (None, groups):
                plan = ops.conv2d_f16s_route(xd, Cout, 1, 1, transposed=True, stats_groups=g)
                assert (plan.route, plan.tup, plan.terms, plan.nimg, plan.fused, plan.part) == (1, row.tup, terms, row.nimg, row.nimg == 1, B), plan
            out = ops.conv_transpose2d_k2s2_f16s(xd, wpk, s, bd, Cout)
            out2, st = ops.conv_transpose2d_k2s2_f16s(xd, wpk, s, bd, Cout, stats_groups=groups)
        o = out[sm].cpu().double()
        outs[terms] = o
        assert torch.equal(out2, out)
        want = ref["y%d" % terms]
        worst[terms] = ratio(o, want, bar)
        assert worst[terms] <= 1.0, ("split-exact", terms, worst[terms])
        if terms == 3:
            assert float((o - ref["true"]).abs().max()) <= 1e-5
        else:
            assert ratio(o, ref["true"], ref["A"]) <= ONE_TERM_BAR
        assert ratio(o, want - ref["d%d" % terms], bar) > 1.0, "a dropped last input channel would pass the bar"
        check_stats(out[sm].cpu(), st, B, groups, sm)
    one_vs_three = ratio(outs[1], ref["y3"], bar)
    assert one_vs_three > 1.0
    print("\nconvT %s worst |out - ref| / (2^-18 A): TERMS=3 %.4f  TERMS=1 %.4f  (one-term vs the three-term bar: %.0f)"
          % (row_id(row), worst[3], worst[1], one_vs_three))
