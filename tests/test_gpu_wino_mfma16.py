"""The 16x16x32 MFMA form of the persistent row-Winograd kernel (csrc/conv_wino.hip: conv_wino_ps_kernel<PRE = 0|1, M16 = 1>), forced with
cf_conv_wino_enable(16), against the split-exact fp64 reference of tests/_split_exact.py at the bars of test_gpu_wino_stream_routes.py.

The form computes the same three split products as the 32x32x16 form with v_mfma_f32_16x16x32_f16: K = 32 is the two 16-channel chunks
of one barrier pair, the V records are the M operand and the weights the N operand, so a lane holds four adjacent units of ONE channel.
The staging waves, the LDS records and the packed weights are those of the 32x32x16 form.  The accumulation order inside a MFMA differs
(32 products per instruction instead of 16), so the outputs are not the bits of level 8; they are held to the same bars:
    |out - y3| <= 2^-18 A per element (SPLIT_BAR, derived in test_gpu_conv_f16s_routes.py; the roundings per accumulator are 4.5 nchunk + 3
    here against 9 nchunk + 3 at level 8), fp64 truth at 2e-5 max(max|y|, 1), the y1 and d3 checks on the output and on the reference alone,
    fused statistics at 2e-6, a repeat run bit-equal; the epilogue at 2e-6 (1 + |pre| + |res|); deferred rows 3e-5 absolute against fp64 and
    2e-5 against the two-pass route.
The form needs an even chunk count per item and whatever the persistent kernel needs; a declined launch runs the kernel that level 8 or
level 1 would run and gives its bits.  ops.wino_mfma (cf_conv2d_wino_mfma) names the shape: 16, 32 or 0; ops.wino_form stays 8.

Row table (pytest -s prints one line per row; the measured table is profiles/wino_mfma16_table.md).
"""
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from _split_exact import ACTS, SPLIT_BAR, TORCH_ACT, check_stats, randn, ratio, wino_split_reference
from test_gpu_wino_stream_routes import (PK_F16S, PK_STREAM, PK_WINO, group_sums, launch_counts, num_cus, prenorm_operands, ps_samples,
                                         wino_forced)

pytestmark = pytest.mark.gpu

Row = namedtuple("Row", "name B C1 C2 H W Cout groups")
ROWS = [
    Row("min16_h8", 2, 32, 0, 8, 16, 128, 8),                 # W == 16, one tile; 2 chunks = one MFMA pair per step
    Row("min32_h8_c224", 2, 64, 0, 8, 32, 224, 8),            # a last block of 96: parked channels in channel block 1 of m-tile 6 and all of 7; groups of 28
    Row("cat20_28_w16", 2, 20, 28, 16, 16, 128, 8),           # concatenation, c1 padded to a chunk: K = 32 spans x1's tail chunk and x2's first
    Row("u480", 2, 480, 0, 16, 16, 480, 480),                 # 30 chunks, four blocks, one group per channel
    Row("unet256", 34, 256, 0, 32, 32, 256, 256),             # 544 items: a workgroup walks several items across samples and channel blocks
]


@pytest.fixture(scope="module")
def case(request, dev):
    from cineflow import ops
    row = request.param
    B, C1, C2, H, W, Cout = row.B, row.C1, row.C2, row.H, row.W, row.Cout
    seed = 11000 + 17 * ROWS.index(row)
    x1 = randn(B, C1, H, W, seed=seed) * 1.3 + 0.2
    x2 = randn(B, C2, H, W, seed=seed + 1) if C2 else None
    w = randn(Cout, C1 + C2, 3, 3, seed=seed + 2) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=seed + 3)
    res = randn(B, Cout, H, W, seed=seed + 4)
    sm = ps_samples(B, H, W, Cout, num_cus(dev))
    xin = x1[sm] if x2 is None else torch.cat([x1[sm], x2[sm]], 1)
    s = ops.pack_conv_weight_wino(w, c1=C1 if C2 else None)[1]
    ref = wino_split_reference(xin, w, b, s)
    bar = SPLIT_BAR * ref["A"]
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0, "the three-term bar does not resolve the lo terms"
    assert ratio(ref["y3"] - ref["d3"], ref["y3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    assert ratio(ref["y3"], ref["true"], ref["A"]) <= 2.0 ** -20
    return dict(row=row, x1=x1, x2=x2, w=w, b=b, res=res, sm=sm, ref=ref, bar=bar)


@pytest.mark.parametrize("case", ROWS, indirect=True, ids=lambda r: r.name)
def test_wino_mfma16_plain(dev, case):
    from cineflow import ops
    c, row = case, case["row"]
    B, C1, C2, H, W, Cout, groups = row.B, row.C1, row.C2, row.H, row.W, row.Cout, row.groups
    sm, ref, bar = c["sm"], c["ref"], c["bar"]
    x1d, x2d = c["x1"].to(dev), None if c["x2"] is None else c["x2"].to(dev)
    wd, bd = c["w"].to(dev), c["b"].to(dev)
    wpk, s = ops.pack_conv_weight_wino(wd, c1=C1 if C2 else None)
    with wino_forced(16):
        assert ops.wino_ok(B, C1, C2, H, W, Cout)
        assert ops.wino_form(B, C1, C2, H, W, Cout) == 8
        assert ops.wino_mfma(B, C1, C2, H, W, Cout) == 16
        with launch_counts() as n:
            out, st = ops.conv2d_wino(x1d, wpk, s, bd, Cout, x2=x2d, stats_groups=groups)
        assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
        again = ops.conv2d_wino(x1d, wpk, s, bd, Cout, x2=x2d)
    o = out[sm].cpu().double()
    worst = ratio(o, ref["y3"], bar)
    scale = max(float(ref["true"].abs().max()), 1.0)
    d = float((o - ref["true"]).abs().max())
    print("\nconv_wino mfma16 %s samples %s: worst |out - y3| / (2^-18 A) = %.4f, max|out - fp64| = %.2e (bar %.2e)" % (row.name, sm, worst, d, 2e-5 * scale))
    assert torch.equal(again, out), "repeat run differs"
    assert worst <= 1.0, ("split-exact", worst)
    assert d <= 2e-5 * scale, ("fp64 contract", d, scale)
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    assert ratio(o, ref["y1"], bar) > 1.0, "the bar does not tell the output from a one-term result"
    check_stats(out[sm].cpu(), st, B, groups, sm)


@pytest.mark.parametrize("case", [ROWS[1]], indirect=True, ids=lambda r: r.name)
def test_wino_mfma16_epilogue(dev, case):
    """alpha, bias, the five activations, a residual and the output slice (channels [2, 2 + Cout) of a sentinel-filled tensor) on the row
    with parked channels, against fp64 act(alpha (y - b) + b) + res of the same form's plain output"""
    from cineflow import ops
    c, row = case, case["row"]
    B, C1, C2, H, W, Cout = row.B, row.C1, row.C2, row.H, row.W, row.Cout
    sm, b = c["sm"], c["b"]
    x1d, bd, resd = c["x1"].to(dev), b.to(dev), c["res"].to(dev)
    wpk, s = ops.pack_conv_weight_wino(c["w"].to(dev))
    with wino_forced(16):
        assert ops.wino_mfma(B, C1, C2, H, W, Cout) == 16
        out = ops.conv2d_wino(x1d, wpk, s, bd, Cout)
        epi = {}
        for act in ACTS:
            big = torch.full((B, Cout + 5, H, W), 7.0, device=dev)
            ops.conv2d_wino(x1d, wpk, s, bd, Cout, act=act, res=resd, out=big, out_coff=2, alpha=0.75)
            assert bool((big[:, :2] == 7.0).all()) and bool((big[:, 2 + Cout:] == 7.0).all()), (act, "sentinel channels written")
            epi[act] = big[sm, 2:2 + Cout].cpu().double()
    o = out[sm].cpu().double()
    bb = b.double().view(1, -1, 1, 1)
    pre = 0.75 * (o - bb) + bb
    rs = c["res"][sm].double()
    for act in ACTS:
        e = TORCH_ACT[act](pre) + rs
        err = float(((epi[act] - e).abs() / (1.0 + pre.abs() + rs.abs())).max())
        print("\nconv_wino mfma16 epilogue %s %s: %.2e (bar 2e-6)" % (row.name, act, err), end="")
        assert err <= 2e-6, (act, err)


def test_wino_mfma16_nonfinite_and_channel_tail(dev):
    """as test_gpu_wino.py: NaN / Inf stay inside their sample, and the zero-weight channel tail of the last chunk (C = 81: 15 padded channels,
    6 chunks) never reads the next sample's first channels"""
    from cineflow import ops
    B, C, H, W, Cout = 2, 81, 32, 32, 128
    x = randn(B, C, H, W, seed=5).to(dev)
    w = (randn(Cout, C, 3, 3, seed=6) / math.sqrt(C * 9)).to(dev)
    wpk, ws = ops.pack_conv_weight_wino(w)
    with wino_forced(16):
        assert ops.wino_mfma(B, C, 0, H, W, Cout) == 16
        clean = ops.conv2d_wino(x, wpk, ws, None, Cout)
        xp = x.clone()
        xp[1, 0] = float("nan")
        out = ops.conv2d_wino(xp, wpk, ws, None, Cout)
        assert torch.equal(out[0], clean[0]) and bool(torch.isnan(out[1]).all())
        xq = x.clone()
        xq[0, 3, 10, 10] = float("inf")
        out = ops.conv2d_wino(xq, wpk, ws, None, Cout)
        assert not bool(torch.isfinite(out[0, :, 10, 10]).any()) and torch.equal(out[1], clean[1])


# deferred normalisation: the persistent rows of test_gpu_wino_stream_routes.WINO_PRE_ROWS with an even chunk count
PreRow = namedtuple("PreRow", "name B C H W Cout gn")
PRE_ROWS = [
    PreRow("c128", 3, 128, 16, 32, 128, 8),
    PreRow("c256_w16", 3, 256, 16, 16, 256, 8),
    PreRow("c480_w16", 2, 480, 16, 16, 480, 8),
]


@pytest.mark.parametrize("row", PRE_ROWS, ids=lambda r: r.name)
def test_wino_mfma16_prenorm(dev, row):
    from cineflow import ops
    B, C, H, W, Cout = row.B, row.C, row.H, row.W, row.Cout
    x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 12000 + 19 * PRE_ROWS.index(row))
    sm = ps_samples(B, H, W, Cout, num_cus(dev))
    xd, gd, btd, bd = x.to(dev), g.to(dev), bt.to(dev), b.to(dev)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    for groups, slope, act, og, cls in ((row.gn, -1.0, "gelu", 8, 2), (C, 0.01, "lrelu", Cout, 1)):
        ws = group_sums(x, groups).to(dev)
        coef = ops.group_norm_coef(ws, gd, btd, groups, B, C, H * W)
        a64 = TORCH_ACT[act](F.group_norm(x[sm].double(), groups, g.double(), bt.double(), eps=1e-5))
        want = F.conv2d(a64, w.double(), b.double(), padding=1)
        with wino_forced(16):
            assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=True) == 8
            assert ops.wino_mfma(B, C, 0, H, W, Cout, prenorm=cls) == 16
            with launch_counts() as n:
                out, st = ops.conv2d_wino_prenorm(xd, coef, slope, wpk, s, bd, Cout, stats_groups=og)
            assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
            applied = ops.group_norm_apply(xd, gd, btd, groups, ws, act=act, out=torch.empty_like(xd))
            two = ops.conv2d_wino(applied, wpk, s, bd, Cout)
            again = ops.conv2d_wino_prenorm(xd, coef, slope, wpk, s, bd, Cout)
        assert torch.equal(again, out), "repeat run differs"
        o = out[sm].cpu().double()
        d, d2 = float((o - want).abs().max()), float((out - two).abs().max())
        print("\nconv_wino mfma16 PRE %s %s: max|out - fp64| = %.2e (bar 3e-5), max|out - two-pass| = %.2e (bar 2e-5), max|y| = %.1f"
              % (row.name, act, d, d2, float(want.abs().max())), end="")
        assert d <= 3e-5, (act, d)
        assert d2 <= 2e-5, (act, d2)
        check_stats(out[sm].cpu(), st, B, og, sm)


def test_wino_mfma16_declines(dev):
    """an odd chunk count, a deferred norm with C % 4 != 0 and a shape outside the family: the query names 32 or 0 and the launch gives
    the bits of the kernel that runs instead (level 8's persistent 32x32x16 form, or the one-tile form that level 1 takes)"""
    from cineflow import ops
    # odd chunk count (C = 48: 3 chunks): the persistent kernel runs with 32x32x16 MFMAs
    B, C, H, W, Cout = 2, 48, 16, 32, 128
    x = randn(B, C, H, W, seed=70).to(dev)
    w = (randn(Cout, C, 3, 3, seed=71) / math.sqrt(C * 9)).to(dev)
    b = randn(Cout, seed=72).to(dev)
    wpk, s = ops.pack_conv_weight_wino(w)
    outs = {}
    for level in (16, 8):
        with wino_forced(level):
            assert ops.wino_form(B, C, 0, H, W, Cout) == 8 and ops.wino_mfma(B, C, 0, H, W, Cout) == 32
            with launch_counts() as n:
                outs[level] = ops.conv2d_wino(x, wpk, s, b, Cout)
            assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
    assert torch.equal(outs[16], outs[8])
    # deferred norm with C % 4 != 0 (C = 81, 6 chunks): the persistent kernel declines, the one-tile form runs as at level 1
    B, C, H, W, Cout = 3, 81, 16, 32, 128
    x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 73)
    xd = x.to(dev)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    coef = ops.group_norm_coef(group_sums(x, 9).to(dev), g.to(dev), bt.to(dev), 9, B, C, H * W)
    outs = {}
    for level in (16, 2):
        with wino_forced(level):
            assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=True) == 2 and ops.wino_mfma(B, C, 0, H, W, Cout, prenorm=2) == 32
            outs[level] = ops.conv2d_wino_prenorm(xd, coef, -1.0, wpk, s, b.to(dev), Cout)
    assert torch.equal(outs[16], outs[2])
    with wino_forced(8):
        assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=True) == 0 and ops.wino_mfma(B, C, 0, H, W, Cout, prenorm=2) == 0
    # outside the family at every level
    with wino_forced(16):
        assert ops.wino_mfma(2, 64, 0, 16, 48, 128) == 0 and not ops.wino_ok(2, 64, 0, 16, 48, 128)
        assert ops.wino_mfma(2, 64, 0, 16, 32, 192) == 0
    # the other levels never name the form on their own account
    for level in (2, 4, 8):
        with wino_forced(level):
            assert ops.wino_mfma(2, 64, 0, 16, 32, 128) == 32


# Level 1 (as shipped): the classes of launch {plain, LeakyReLU-deferred, GELU-deferred} x {TW 32, TW 16} that the decision table of
# conv_wino.hip (WINO_M16_CLASS) sends to the form -- one bench layer shape per class, the batch reduced to two items per CU.  The table
# here restates the kernel's; a class moves in both places, with its measurement (profiles/wino_mfma16_bench.md).
LEVEL1_M16 = {(0, 32): True, (0, 16): True, (1, 32): True, (1, 16): True, (2, 32): True, (2, 16): False}
L1Row = namedtuple("L1Row", "name cls C H W Cout")
L1_ROWS = [
    L1Row("plain_128x128_c128", 0, 128, 128, 128, 128),      # 128 tiles per sample
    L1Row("plain_16x16_c480", 0, 480, 16, 16, 480),          # 2 tiles x 4 blocks per sample
    L1Row("lrelu_64x64_c128", 1, 128, 64, 64, 128),          # 32 tiles per sample
    L1Row("lrelu_16x16_c480", 1, 480, 16, 16, 480),
    L1Row("gelu_128x128_c128", 2, 128, 128, 128, 128),
    L1Row("gelu_16x16_c256", 2, 256, 16, 16, 256),           # 2 tiles x 2 blocks per sample
]


@pytest.mark.parametrize("row", L1_ROWS, ids=lambda r: r.name)
def test_wino_mfma16_level1(dev, row):
    from cineflow import ops
    C, H, W, Cout, cls = row.C, row.H, row.W, row.Cout, row.cls
    TW, TH = (32, 4) if W >= 32 else (16, 8)
    per = (W // TW) * (H // TH) * ((Cout + 127) // 128)
    B = -(-2 * num_cus(dev) // per)                                     # just two items per CU
    x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 13000 + 7 * L1_ROWS.index(row))
    xd, bd = x.to(dev), b.to(dev)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    want = 16 if LEVEL1_M16[(cls, TW)] else 32
    with wino_forced(1):
        assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=cls != 0) == 8
        assert ops.wino_mfma(B, C, 0, H, W, Cout, prenorm=cls) == want, "level 1 routes this class otherwise than the table says"
        with launch_counts() as n:
            if cls == 0:
                out = ops.conv2d_wino(xd, wpk, s, bd, Cout)
            else:
                groups = 8 if cls == 2 else C
                coef = ops.group_norm_coef(group_sums(x, groups).to(dev), g.to(dev), bt.to(dev), groups, B, C, H * W)
                out = ops.conv2d_wino_prenorm(xd, coef, -1.0 if cls == 2 else 0.01, wpk, s, bd, Cout)
        assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
    with wino_forced(16 if want == 16 else 8):                          # the level that forces the same kernel gives the same bits
        if cls == 0:
            forced = ops.conv2d_wino(xd, wpk, s, bd, Cout)
        else:
            forced = ops.conv2d_wino_prenorm(xd, coef, -1.0 if cls == 2 else 0.01, wpk, s, bd, Cout)
    assert torch.equal(out, forced)
