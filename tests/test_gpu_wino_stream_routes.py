"""Every instantiation of the row-Winograd kernels (csrc/conv_wino.hip: conv_wino_kernel<NTW = 2|4, PRE = 0|1>, conv_wino_ps_kernel<PRE = 0|1, M16 = 0|1>)
and of the persistent pipelined kernel (csrc/conv_stream.hip: conv_stream_kernel<WM = 1|2, PRE = 0|1>) against a split-exact fp64 reference,
per output element, at the geometry edges of each form.  No row skips: a row names the forms that must take it, forces each with
cf_conv_wino_enable(2 | 4 | 8) / cf_conv_stream_enable(2) and asserts the routing (ops.wino_ok and ops.wino_form; the launch counters of cf_profile_read
tell which family took a launch, a rocprofv3 kernel trace read by tools/kernel_coverage.py tells which instantiation).

Which form takes which map (wino_geometry / wino_plan, the one plan the probes read and the launch executes).  W must be 16 or a multiple of 32.  W >= 32: tiles of 32 columns x TH rows with
TH = 4 (NTW 2 and the persistent kernel) or 8 (NTW 4); W == 16: 16 columns x TH = 8 (NTW 2, persistent) or 16 (NTW 4).  H must be a multiple
of TH; the staging-task and LDS budgets hold for all of these.  Level 1 (as shipped) takes the persistent kernel from 2 x CUs items (tiles x
samples x 128-channel blocks), else NTW 2: wino_plan never chooses NTW 4 by itself, so conv_wino_kernel<4, *> runs only under the
forced level 4 (CF_CONV_WINO=4 / cf_conv_wino_enable(4)) -- a kernel that is built and tested here but that no shipped route reaches.
ops.wino_form (cf_conv2d_wino_form) returns the form the dispatch picks; every row asserts it.  The persistent kernel declines a deferred
normalisation with C % 4 != 0.
conv_stream takes 3x3 / stride 1 layers to 32 (WM 1, tiles of 16 rows) or 64 (WM 2, 8 rows) channels written plainly, W % 4 == 0, W >= 32,
H >= 16, an even number of 16-channel chunks and at least 1024 tiles of 32 columns.

Winograd reference (tests/_split_exact.py: wino_split_reference; checked against an fp64 convolution on the CPU in
test_split_exact_reference.py).  The kernel's operands are reproducible exactly: the input transform is one fp32 operation per value,
done before the split, and the weights are transformed on the host:
    V[ci][row][u][0..3] = fp32(d0 - d2, d1 + d2, d2 - d1, d1 - d3),  d = x[row][2u - 1 .. 2u + 2], zero outside the image
    Vh = fp16(V), Vl = fp16(V - Vh);   us = fp32(2^s G w) (pack_conv_weight_wino), Uh = fp16(us), Ul = fp16(us - Uh)
    M_j = sum over (ci, ky) of Uh Vh + Uh Vl + Ul Vh   (float64, rows zero padded),  j = 0..3
    y3[2u] = 2^-s (M0 + M1 + M2) + b,  y3[2u + 1] = 2^-s (M1 - M2 - M3) + b;    y1: the Uh Vh term alone
    A[2u]  = 2^-s (A0 + A1 + A2) + |b|, A[2u + 1] = 2^-s (A1 + A2 + A3) + |b|,  A_j = sum (|Uh| + |Ul|)(|Vh| + |Vl|)
A product of two fp16 values is exact in fp32, so the kernel differs from y3 only by the rounding of its fp32 accumulation, the two
additions of the output transform and the epilogue's alpha * acc + b.  conv_stream multiplies the operands of conv_f16s (same packed
weights): split_reference of the f16s module applies unchanged.

Bar: 2^-18 A per output element, the project's SPLIT_BAR (derived in test_gpu_conv_f16s_routes.py: with unit roundoff u = 2^-24 the
deterministic bound is (n + 1) u A for n roundings, certain below the bar for n <= 63; as a random walk the error grows like sqrt(n) u A and
stays below 64 u A up to n ~ 4000).  The Winograd accumulators see n = 9 nchunk + 3 roundings (three products x three ky per chunk and
position, the output transform, the epilogue): 21 at 32 channels, 84 at 144, 543 at 960 -- every row from 7 chunks up rests on the
random-walk half of that derivation, not on the certain one.  conv_stream: n = 27 nchunk + 1 (<= 163 here).  The bar is not fitted to the
kernels: a correct-looking kernel above it would be a finding to explain.  Worst measured ratio to the bar per row: pytest -s.
Measured on the MI355X (worst over all rows of a family): conv_wino 0.029 of the bar (cat20_28_w16; the one-tile forms and the persistent
kernel accumulate in the same order and gave the same bits on every row, so the figure is one for conv_wino_kernel and
conv_wino_ps_kernel alike; 0.024 at 960 channels), conv_stream 0.056 (<2,0> at 256 x 256).

Each plain row also proves on the reference alone that the bar can fail (y1, and y3 without the split-exact contribution of the last input
channel, both miss the bar against y3), keeps the suite's older contract (fp64 convolution of the true operands at 2e-5 max(max|y|, 1) for
Winograd, 1e-5 for conv_stream; <= 1e-5 of that scale against conv2d_f16s on the same operands, 4e-6 (1 + max|y|) for conv_stream, whose
repeat runs are bit-equal), checks the fused GroupNorm statistics against fp64 sums of the stored output at 2e-6, and -- Winograd, whose
epilogue is its own -- runs all five activations with alpha = 0.75 and a residual into channels [2, 2 + Cout) of a tensor filled with a
sentinel, against fp64 act(alpha (y - b) + b) + res of the same launch's plain output at 2e-6 (1 + |pre| + |res|).  conv_stream has no
epilogue of its own: with an activation, a residual or an output slice it must decline (asserted bit for bit against level 0).

PRE rows (deferred GroupNorm(8) + GELU and InstanceNorm + LeakyReLU, per-sample statistics made different on purpose) normalise in fp32
inside the kernel, so the split-exact reference does not apply: fp64 at 3e-5 absolute and 2e-5 against the two-pass route (group_norm_apply,
then the same kernel family on the materialised activation), the bars of the f16s module's PRE rows; conv_stream PRE keeps its tighter 2e-5
against fp64 and 4e-6 (1 + max|y|) against conv_f16s' PRE kernel.

Large rows compare selected samples against the CPU reference: the first and the last, for conv_stream a middle one, and for persistent
Winograd launches with more items than workgroups the samples of the first two items of workgroup 0 (either side of the first item
boundary of its chunk stream) and the sample of the second item of the last band's first workgroup.
"""
import contextlib
import ctypes
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from _split_exact import (ACTS, SPLIT_BAR, TORCH_ACT, check_stats, device_input, randn, ratio, split_reference, wino_split_reference)

pytestmark = pytest.mark.gpu

PK_F16S, PK_STREAM, PK_WINO = 6, 15, 16


@contextlib.contextmanager
def wino_forced(level):
    from cineflow._lib import lib
    prev = lib().cf_conv_wino_enable(level)
    try:
        yield
    finally:
        lib().cf_conv_wino_enable(prev)


@contextlib.contextmanager
def stream_forced(level):
    from cineflow._lib import lib
    prev = lib().cf_conv_stream_enable(level)
    try:
        yield
    finally:
        lib().cf_conv_stream_enable(prev)


@contextlib.contextmanager
def launch_counts():
    """{kernel id: launches} of the three convolution families for the calls made inside (filled on exit)"""
    from cineflow._lib import check, lib
    h = lib()
    got = {}
    check(h.cf_profile_enable(64), "cf_profile_enable")
    try:
        yield got
        torch.cuda.synchronize()
        for kid in (PK_F16S, PK_STREAM, PK_WINO):
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
            check(h.cf_profile_read(kid, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)), "cf_profile_read")
            got[kid] = n.value
    finally:
        check(h.cf_profile_enable(0), "cf_profile_enable")


def num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def wino_tile(level, W):
    """(TW, TH) of a form (2, 4: one tile per workgroup; 8: persistent, the geometry of NTW 2)"""
    ntw = 4 if level == 4 else 2
    return (32, 2 * ntw) if W >= 32 else (16, 4 * ntw)


def ps_samples(B, H, W, Cout, ncu):
    """samples worth comparing on a persistent launch (conv_wino_ps_kernel's item walk: item = block * ntiles + tile, eight bands, workgroup
    wgi of a band takes items band_lo + wgi + i * nwg / 8): the first and the last, and where workgroups walk several items the samples of
    workgroup 0's first two items (either side of the first item boundary of its stream) and of the second item of the last band's first
    workgroup.  This restates the kernel's walk: a change of the walk must be followed here."""
    TW, TH = wino_tile(8, W)
    per = (W // TW) * (H // TH)
    ntiles = per * B
    nitems = ntiles * ((Cout + 127) // 128)
    nwgx = min(ncu, (nitems + 7) & ~7) // 8
    s = {0, B - 1}
    if nwgx < nitems // 8:                                   # the first workgroup of every band has a second item
        s |= {(i % ntiles) // per for i in (0, nwgx, nitems * 7 // 8 + nwgx)}
    return sorted(s)


def auto_form(B, H, W, Cout, ncu):
    """what wino_plan does at route level 1 for a plain layer: the persistent kernel from two items per CU, else NTW 2 (never NTW 4)"""
    TW, TH = wino_tile(2, W)
    if W % TW or H % TH:
        return 0
    return 8 if (W // TW) * (H // TH) * B * ((Cout + 127) // 128) >= 2 * ncu else 2


# ------------------------------------------------------------------------------------------------------------------ Winograd, plain
# forms: the route levels that must take the row (2 / 4: conv_wino_kernel<NTW, 0>, 8: conv_wino_ps_kernel<0, 0>); every other level must decline
# it (test_wino_forms_decline_what_their_geometry_forbids).  groups: fused statistics groups.  All five activations (the ConvGRU gates'
# sigmoid at Cout = 512 among them), alpha, residual and the sentinel-fenced slice run on every row.
WRow = namedtuple("WRow", "name forms B C1 C2 H W Cout groups")
WINO_ROWS = [
    # ---- smallest maps: one tile holds all four image borders
    WRow("min16_h8", (2, 8), 2, 32, 0, 8, 16, 128, 8),               # W == 16, H == TH == 8 of NTW 2 / persistent; NTW 4 needs H % 16 == 0
    WRow("min16_h16", (2, 4, 8), 2, 48, 0, 16, 16, 256, 8),          # W == 16, H == TH == 16 of NTW 4 (two tile rows for the others); 3 chunks
    WRow("min32_h4", (2, 8), 3, 32, 0, 4, 32, 128, 128),             # W == 32, H == TH == 4 of NTW 2 / persistent; NTW 4 needs H % 8 == 0
    WRow("min32_h8_c224", (2, 4, 8), 2, 64, 0, 8, 32, 224, 8),       # W == 32, H == TH == 8 of NTW 4; 224 = 128 + 96: parked channels, groups of 28
    # ---- tile grid edges
    WRow("w96", (2, 4, 8), 2, 40, 0, 8, 96, 128, 8),                 # three tile columns (odd); 40 channels: half a chunk of tail
    WRow("w16_rows_c480", (2, 4, 8), 2, 64, 0, 32, 16, 480, 480),    # W == 16 with 4 (2) tile rows; 480 = 3 x 128 + 96, one group per channel
    WRow("h12", (2, 8), 2, 32, 0, 12, 32, 128, 8),                   # H % 8 != 0: NTW 4 declines
    # ---- output widths
    WRow("c512_gates", (2, 4, 8), 2, 128, 128, 16, 32, 512, 8),      # ConvGRU gates: cat[h, x] -> 512 (sigmoid runs with the other activations)
    WRow("c256", (2, 4, 8), 2, 81, 0, 16, 64, 256, 8),               # single input with a channel tail (81 = 5 chunks + 1)
    # ---- two inputs, split not a chunk multiple (split-aware packing: x1's channels padded to whole chunks)
    WRow("cat100_60", (2, 4, 8), 1, 100, 60, 32, 64, 224, 8),
    WRow("cat20_28_w16", (2, 4, 8), 2, 20, 28, 16, 16, 480, 480),
    # ---- 960 input channels (the U-Net decoder's cat[skip, up] at 16 x 16): 60 chunks, n = 543 roundings
    WRow("c960", (2, 4, 8), 2, 480, 480, 16, 16, 480, 480),
    # ---- persistent kernel with more items than workgroups: 2 tiles x 4 blocks x 40 samples = 320 items; workgroups 0..7 of each band walk two
    WRow("ps320_odd", (2, 4, 8), 40, 144, 0, 16, 16, 480, 480),      # 9 chunks per item: odd streams, the padded last pair
    WRow("ps320_even", (2, 4, 8), 40, 128, 0, 16, 16, 480, 8),       # 8 chunks per item; 8 groups of 60 across the 32-channel m-tiles
]
WINO_PARAMS = [pytest.param(r, lv, id="%s-L%d" % (r.name, lv)) for r in WINO_ROWS for lv in r.forms]


@pytest.fixture(scope="module")
def wino_case(request, dev):
    """operands, the samples compared and the CPU reference of a row (request.param), built once and shared by the row's forms"""
    from cineflow import ops
    row = request.param
    B, C1, C2, H, W, Cout = row.B, row.C1, row.C2, row.H, row.W, row.Cout
    seed = 1000 + 17 * WINO_ROWS.index(row)
    x1 = randn(B, C1, H, W, seed=seed) * 1.3 + 0.2
    x2 = randn(B, C2, H, W, seed=seed + 1) if C2 else None
    w = randn(Cout, C1 + C2, 3, 3, seed=seed + 2) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=seed + 3)
    res = randn(B, Cout, H, W, seed=seed + 4)
    sm = ps_samples(B, H, W, Cout, num_cus(dev)) if 8 in row.forms else [0, B - 1]
    xin = x1[sm] if x2 is None else torch.cat([x1[sm], x2[sm]], 1)
    s = ops.pack_conv_weight_wino(w, c1=C1 if C2 else None)[1]
    ref = wino_split_reference(xin, w, b, s)
    bar = SPLIT_BAR * ref["A"]
    # the bar can fail, on the reference alone
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0, "the three-term bar does not resolve the lo terms"
    assert ratio(ref["y3"] - ref["d3"], ref["y3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    assert ratio(ref["y3"], ref["true"], ref["A"]) <= 2.0 ** -20
    return dict(row=row, x1=x1, x2=x2, w=w, b=b, res=res, sm=sm, ref=ref, bar=bar)


@pytest.mark.parametrize("wino_case,level", WINO_PARAMS, indirect=["wino_case"])
def test_conv_wino_route(dev, wino_case, level):
    from cineflow import ops
    c, row = wino_case, wino_case["row"]
    B, C1, C2, H, W, Cout, groups = row.B, row.C1, row.C2, row.H, row.W, row.Cout, row.groups
    sm, ref, bar, b = c["sm"], c["ref"], c["bar"], c["b"]
    if row.name.startswith("ps320"):                                # 320 items on 256 workgroups: samples 0 | 16 (workgroup 0), 36 (band 7), 39
        assert 320 > num_cus(dev) and len(sm) == 4, "the row is meant to give workgroups a second item"
    x1d, x2d = c["x1"].to(dev), None if c["x2"] is None else c["x2"].to(dev)
    wd, bd, resd = c["w"].to(dev), b.to(dev), c["res"].to(dev)
    wpk, s = ops.pack_conv_weight_wino(wd, c1=C1 if C2 else None)
    with wino_forced(level):
        assert ops.wino_ok(B, C1, C2, H, W, Cout), "route level %d no longer takes this shape" % level
        assert ops.wino_form(B, C1, C2, H, W, Cout) == level
        with launch_counts() as n:
            out, st = ops.conv2d_wino(x1d, wpk, s, bd, Cout, x2=x2d, stats_groups=groups)
        assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
        epi = {}
        for act in ACTS:
            big = torch.full((B, Cout + 5, H, W), 7.0, device=dev)
            ops.conv2d_wino(x1d, wpk, s, bd, Cout, x2=x2d, act=act, res=resd, out=big, out_coff=2, alpha=0.75)
            assert bool((big[:, :2] == 7.0).all()) and bool((big[:, 2 + Cout:] == 7.0).all()), (act, "sentinel channels written")
            epi[act] = big[sm, 2:2 + Cout].cpu().double()
        again = ops.conv2d_wino(x1d, wpk, s, bd, Cout, x2=x2d)
    assert torch.equal(again, out), "repeat run differs"
    o = out[sm].cpu().double()
    worst = ratio(o, ref["y3"], bar)
    print("\nconv_wino %s level %d samples %s: worst |out - y3| / (2^-18 A) = %.4f" % (row.name, level, sm, worst))
    assert worst <= 1.0, ("split-exact", worst)
    scale = max(float(ref["true"].abs().max()), 1.0)
    d = float((o - ref["true"]).abs().max())
    assert d <= 2e-5 * scale, ("fp64 contract", d, scale)
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    assert ratio(o, ref["y1"], bar) > 1.0, "the bar does not tell the output from a one-term result"
    with wino_forced(0):                                             # the direct kernel on the same operands, every sample
        wpd, sd = ops.pack_conv_weight_f16s(wd, c1=C1 if (C2 and C1 % 16) else None)
        direct = ops.conv2d_f16s(x1d, wpd, sd, bd, Cout, 3, 3, 1, (1, 1), x2=x2d)
    assert float((out - direct).abs().max()) <= 1e-5 * scale
    check_stats(out[sm].cpu(), st, B, groups, sm)
    bb = b.double().view(1, -1, 1, 1)
    pre = 0.75 * (o - bb) + bb
    rs = c["res"][sm].double()
    for act in ACTS:
        e = TORCH_ACT[act](pre) + rs
        err = float(((epi[act] - e).abs() / (1.0 + pre.abs() + rs.abs())).max())
        assert err <= 2e-6, (act, err)


def test_wino_forms_decline_what_their_geometry_forbids(dev):
    """the complement of the table: a forced form whose tile rows do not divide H declines, and so does every form where W is neither 16 nor
    a multiple of 32, or H no multiple of the smallest tile"""
    from cineflow import ops
    for row in WINO_ROWS:
        for level in (2, 4, 8):
            TW, TH = wino_tile(level, row.W)
            assert (level in row.forms) == (row.W % TW == 0 and row.H % TH == 0), (row.name, level)     # the table agrees with the geometry
            with wino_forced(level):
                assert ops.wino_ok(row.B, row.C1, row.C2, row.H, row.W, row.Cout) == (level in row.forms), (row.name, level)
    for level in (1, 2, 4, 8):
        with wino_forced(level):
            assert not ops.wino_ok(2, 64, 0, 16, 48, 128), "W = 48: not a multiple of the 32-column tile"
            assert not ops.wino_ok(2, 64, 0, 10, 32, 128), "H = 10: no multiple of 4"
            assert not ops.wino_ok(2, 64, 0, 12, 16, 128), "H = 12 at W = 16: no multiple of 8"
            assert not ops.wino_ok(2, 64, 64, 16, 32, 128, prenorm=True), "deferred normalisation: single input only"
            assert not ops.wino_ok(2, 64, 0, 16, 32, 192), "192 = 128 + 64: last block under three quarters"
    with wino_forced(8):                                             # the persistent kernel loads the coefficient quads of 4 channels at once
        assert not ops.wino_ok(2, 81, 0, 16, 32, 128, prenorm=True) and ops.wino_ok(2, 84, 0, 16, 32, 128, prenorm=True)
    with wino_forced(1):                                             # ... and as shipped such a layer runs on NTW 2, however many items it has
        assert ops.wino_ok(2, 81, 0, 16, 32, 128, prenorm=True)
        assert ops.wino_form(2, 81, 0, 16, 32, 128, prenorm=True) == 2 and ops.wino_form(600, 81, 0, 16, 32, 128, prenorm=True) == 2
        assert ops.wino_form(600, 84, 0, 16, 32, 128, prenorm=True) == 8


# ---- the production choice (route level 1) at the bench's layer shapes, batch reduced.  The expected form is derived from the CU count by
# auto_form (the comments give it for the MI355X's 256 CUs) and held against ops.wino_form, the dispatch's own answer for the shape; the
# launch counters show that the Winograd family took the call, the kernel trace which instantiation.  The forms give the same bits (same
# accumulation order), so comparing outputs cannot tell them apart.  Level 1 never takes NTW 4, whatever the geometry allows.
AutoRow = namedtuple("AutoRow", "name B C1 C2 H W Cout groups")
AUTO_ROWS = [
    AutoRow("enc128", 4, 128, 0, 128, 128, 128, 8),        # flow encoder: 128 tiles x 4 samples = 512 items = 2 x 256 CUs -> persistent
    AutoRow("unet256", 34, 256, 0, 32, 32, 256, 256),      # U-Net stage: 8 tiles x 2 blocks x 34 = 544 items -> persistent
    AutoRow("enc128_b3", 3, 128, 0, 128, 128, 128, 8),     # 384 items, just under 2 x 256 -> NTW 2
    AutoRow("enc256", 2, 256, 0, 64, 64, 256, 8),          # 128 items -> NTW 2, although H % 8 == 0 would admit NTW 4
    AutoRow("dec480", 2, 480, 480, 16, 16, 480, 480),      # 16 items, W == 16 -> NTW 2, although H % 16 == 0 would admit NTW 4
    AutoRow("h12", 2, 128, 0, 12, 32, 128, 8),             # 6 items, H % 8 != 0 -> NTW 2
]


@pytest.mark.parametrize("row", AUTO_ROWS, ids=lambda r: r.name)
def test_conv_wino_route_as_shipped(dev, row):
    from cineflow import ops
    from cineflow.nn import Conv2d
    B, C1, C2, H, W, Cout, groups = row.B, row.C1, row.C2, row.H, row.W, row.Cout, row.groups
    ncu = num_cus(dev)
    form = auto_form(B, H, W, Cout, ncu)
    assert form in (2, 8)
    seed = 3000 + 13 * AUTO_ROWS.index(row)
    x1 = randn(B, C1, H, W, seed=seed)
    x2 = randn(B, C2, H, W, seed=seed + 1) if C2 else None
    w = randn(Cout, C1 + C2, 3, 3, seed=seed + 2) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=seed + 3)
    sm = ps_samples(B, H, W, Cout, ncu) if form == 8 else [0, B - 1]
    m = Conv2d(C1 + C2, Cout, 3, padding=1)
    m.load_state_dict({"weight": w, "bias": b}, dev)
    x1d, x2d = x1.to(dev), None if x2 is None else x2.to(dev)
    with wino_forced(1):
        assert ops.wino_ok(B, C1, C2, H, W, Cout)
        assert ops.wino_form(B, C1, C2, H, W, Cout) == form, "level 1 picks another form than documented for %d CUs" % ncu
        with launch_counts() as n:
            out, st = m(x1d, x2d, stats_groups=groups)
        assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
    s = ops.pack_conv_weight_wino(w, c1=C1 if C2 else None)[1]
    ref = wino_split_reference(x1[sm] if x2 is None else torch.cat([x1[sm], x2[sm]], 1), w, b, s)
    bar = SPLIT_BAR * ref["A"]
    o = out[sm].cpu().double()
    worst = ratio(o, ref["y3"], bar)
    print("\nconv_wino as shipped %s (form %d) samples %s: worst |out - y3| / (2^-18 A) = %.4f" % (row.name, form, sm, worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0 and ratio(ref["y3"] - ref["d3"], ref["y3"], bar) > 1.0
    assert float((o - ref["true"]).abs().max()) <= 2e-5 * max(float(ref["true"].abs().max()), 1.0)
    check_stats(out[sm].cpu(), st, B, groups, sm)


# ------------------------------------------------------------------------------------------------------------------ Winograd, PRE
# deferred normalisation: conv_wino_kernel<NTW, 1>, conv_wino_ps_kernel<1, 0>.  gn: groups of the GroupNorm + GELU pass (8 where C % 8 == 0).
PreRow = namedtuple("PreRow", "name forms B C H W Cout gn")
WINO_PRE_ROWS = [
    PreRow("c128", (2, 4, 8), 3, 128, 16, 32, 128, 8),
    PreRow("c256_w16", (2, 4, 8), 3, 256, 16, 16, 256, 8),            # 16-wide maps
    PreRow("c480_w16", (2, 4, 8), 2, 480, 16, 16, 480, 8),            # 480 -> 480: parked output channels
    PreRow("c104_w96", (2, 4, 8), 3, 104, 8, 96, 224, 8),             # 104 = 6 chunks + 8: C % 16 != 0, C % 4 == 0 -> the persistent kernel takes it
    PreRow("c81", (2, 4), 3, 81, 16, 32, 128, 9),                     # C % 4 != 0: the persistent kernel declines, the coefficient tail c < C1 ? .. : 0
    PreRow("ps320_c100", (2, 4, 8), 40, 100, 16, 16, 480, 4),         # 320 items: coefficient quads follow the stream across samples; 7 chunks (odd)
]
WINO_PRE_PARAMS = [pytest.param(r, lv, id="%s-L%d" % (r.name, lv)) for r in WINO_PRE_ROWS for lv in r.forms]


def prenorm_operands(B, C, H, W, Cout, seed):
    k = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    x = randn(B, C, H, W, seed=seed) * (1.0 + 0.2 * k) + 0.1 * k - 0.3          # per-sample statistics differ
    g, bt = 1 + 0.3 * randn(C, seed=seed + 1), 0.3 * randn(C, seed=seed + 2)
    w = randn(Cout, C, 3, 3, seed=seed + 3) / math.sqrt(C * 9)
    b = randn(Cout, seed=seed + 4)
    return x, g, bt, w, b


def group_sums(x, groups):
    xs = x.double().view(x.shape[0], groups, -1)
    return torch.stack([xs.sum(-1), (xs ** 2).sum(-1)], -1).reshape(-1)


@pytest.mark.parametrize("row,level", WINO_PRE_PARAMS)
def test_conv_wino_prenorm_route(dev, row, level):
    from cineflow import ops
    B, C, H, W, Cout = row.B, row.C, row.H, row.W, row.Cout
    x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 5000 + 19 * WINO_PRE_ROWS.index(row))
    sm = ps_samples(B, H, W, Cout, num_cus(dev)) if 8 in row.forms else [0, B - 1]
    xd, gd, btd, bd = x.to(dev), g.to(dev), bt.to(dev), b.to(dev)
    wpk, s = ops.pack_conv_weight_wino(w.to(dev))
    for groups, slope, act, og in ((row.gn, -1.0, "gelu", 8), (C, 0.01, "lrelu", Cout)):
        ws = group_sums(x, groups).to(dev)
        coef = ops.group_norm_coef(ws, gd, btd, groups, B, C, H * W)
        a64 = TORCH_ACT[act](F.group_norm(x[sm].double(), groups, g.double(), bt.double(), eps=1e-5))
        want = F.conv2d(a64, w.double(), b.double(), padding=1)
        with wino_forced(level):
            assert ops.wino_ok(B, C, 0, H, W, Cout, prenorm=True), "route level %d no longer takes this shape" % level
            assert ops.wino_form(B, C, 0, H, W, Cout, prenorm=True) == level
            with launch_counts() as n:
                out, st = ops.conv2d_wino_prenorm(xd, coef, slope, wpk, s, bd, Cout, stats_groups=og)
            assert n == {PK_WINO: 1, PK_F16S: 0, PK_STREAM: 0}, n
            applied = ops.group_norm_apply(xd, gd, btd, groups, ws, act=act, out=torch.empty_like(xd))
            two = ops.conv2d_wino(applied, wpk, s, bd, Cout)
            again = ops.conv2d_wino_prenorm(xd, coef, slope, wpk, s, bd, Cout)
        assert torch.equal(again, out), "repeat run differs"
        o = out[sm].cpu().double()
        d, d2 = float((o - want).abs().max()), float((out - two).abs().max())
        print("\nconv_wino PRE %s level %d %s: max|out - fp64| = %.2e (bar 3e-5), max|out - two-pass| = %.2e (bar 2e-5), max|y| = %.1f"
              % (row.name, level, act, d, d2, float(want.abs().max())), end="")
        assert d <= 3e-5, (act, d)
        assert d2 <= 2e-5, (act, d2)
        check_stats(out[sm].cpu(), st, B, og, sm)


# ------------------------------------------------------------------------------------------------------------------ conv_stream
# conv_stream_kernel<WM, PRE>: Cout = 32 WM; tiles of 32 columns x 16 (WM 1) or 8 (WM 2) rows; ntiles = B x ceil(H / TH) x ceil(W / 32) >= 1024
SRow = namedtuple("SRow", "name WM PRE B C1 C2 H W ntiles")
STREAM_ROWS = [
    SRow("bench", 1, 0, 8, 32, 0, 256, 256, 1024),              # Generic_UNet level 0
    SRow("ragged", 1, 0, 171, 32, 0, 40, 44, 1026),             # H = 2.5 tiles, W = 32 + 12; 1026 tiles: bands of 128 and 129
    SRow("min", 1, 0, 1027, 32, 0, 16, 32, 1027),               # the minimum map: one tile per sample, the tile count from B alone, bands unequal
    SRow("tail81", 1, 0, 257, 81, 0, 32, 64, 1028),             # 6 chunks, 15 zero-weight channels
    SRow("cat20_28", 1, 0, 257, 20, 28, 32, 64, 1028),          # two inputs, a padded tail behind each
    SRow("bench", 2, 0, 4, 64, 0, 256, 256, 1024),              # flow decoder at level 0
    SRow("ragged", 2, 0, 171, 32, 0, 20, 44, 1026),             # H = 2.5 tiles
    SRow("min", 2, 0, 513, 32, 0, 16, 32, 1026),                # two tiles per sample
    SRow("tail81", 2, 0, 129, 81, 0, 32, 64, 1032),
    SRow("cat20_28", 2, 0, 129, 20, 28, 32, 64, 1032),
    SRow("bench", 1, 1, 8, 32, 0, 256, 256, 1024),              # Generic_UNet level 0, second convolution
    SRow("ragged", 1, 1, 171, 32, 0, 40, 44, 1026),
    SRow("min", 1, 1, 1027, 32, 0, 16, 32, 1027),
    SRow("tail24", 1, 1, 257, 24, 0, 32, 64, 1028),             # two chunks, eight padded channels: the coefficient table's tail
    SRow("bench", 2, 1, 4, 64, 0, 256, 256, 1024),              # only level 2 of the knob sends 64-channel PRE layers here
    SRow("ragged", 2, 1, 171, 32, 0, 20, 44, 1026),
    SRow("min", 2, 1, 513, 32, 0, 16, 32, 1026),
    SRow("tail24", 2, 1, 129, 24, 0, 32, 64, 1032),
]


def srow_id(r):
    return "<%d,%d>_%s" % (r.WM, r.PRE, r.name)


def stream_tiles(r):
    TH = 16 if r.WM == 1 else 8
    return r.B * ((r.H + TH - 1) // TH) * ((r.W + 31) // 32)


@pytest.mark.parametrize("row", [r for r in STREAM_ROWS if not r.PRE], ids=srow_id)
def test_conv_stream_route(dev, row):
    from cineflow import ops
    B, C1, C2, H, W, Cout = row.B, row.C1, row.C2, row.H, row.W, 32 * row.WM
    assert stream_tiles(row) == row.ntiles >= 1024
    seed = 7000 + 23 * STREAM_ROWS.index(row)
    x1 = randn(B, C1, H, W, seed=seed) * 1.3 + 0.2
    x2 = randn(B, C2, H, W, seed=seed + 1) if C2 else None
    w = randn(Cout, C1 + C2, 3, 3, seed=seed + 2) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=seed + 3)
    groups = 8 if row.WM == 2 else 32
    sm = [0, B // 2, B - 1]
    x1d, x2d, bd = x1.to(dev), None if x2 is None else x2.to(dev), b.to(dev)
    wpk, s = ops.pack_conv_weight_f16s(w.to(dev), c1=C1 if (C2 and C1 % 16) else None)
    args = (x1d, wpk, s, bd, Cout, 3, 3, 1, (1, 1))
    with stream_forced(2):
        with launch_counts() as n:
            out, st = ops.conv2d_f16s(*args, x2=x2d, stats_groups=groups)
        assert n == {PK_STREAM: 1, PK_F16S: 0, PK_WINO: 0}, ("conv_stream did not take the layer", n)
        plain = ops.conv2d_f16s(*args, x2=x2d)
        again, st2 = ops.conv2d_f16s(*args, x2=x2d, stats_groups=groups)
    with stream_forced(0):
        with launch_counts() as n:
            ref_out = ops.conv2d_f16s(*args, x2=x2d)
        assert n == {PK_STREAM: 0, PK_F16S: 1, PK_WINO: 0}, n
    assert torch.equal(again, out) and torch.equal(plain, out), "repeat run differs"
    assert float((out - ref_out).abs().max()) <= 4e-6 * (1.0 + float(ref_out.abs().max()))
    xin = x1[sm] if x2 is None else torch.cat([x1[sm], x2[sm]], 1)
    ref = split_reference(xin, w, b, s, lambda a, m: F.conv2d(a, m, padding=1))
    bar = SPLIT_BAR * ref["A"]
    o = out[sm].cpu().double()
    worst = ratio(o, ref["y3"], bar)
    print("\nconv_stream %s samples %s: worst |out - y3| / (2^-18 A) = %.4f" % (srow_id(row), sm, worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert float((o - ref["true"]).abs().max()) <= 1e-5, "fp64 contract"
    assert ratio(ref["y1"], ref["y3"], bar) > 1.0, "the three-term bar does not resolve the lo terms"
    assert ratio(o, ref["y1"], bar) > 1.0, "the bar does not tell the output from a one-term result"
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    for s_ in (st, st2):
        check_stats(out[sm].cpu(), s_, B, groups, sm)


@pytest.mark.parametrize("row", [r for r in STREAM_ROWS if r.PRE], ids=srow_id)
def test_conv_stream_prenorm_route(dev, row):
    from cineflow import ops
    B, C, H, W, Cout = row.B, row.C1, row.H, row.W, 32 * row.WM
    assert stream_tiles(row) == row.ntiles >= 1024
    x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 9000 + 29 * STREAM_ROWS.index(row))
    sm = [0, B // 2, B - 1]
    xd, gd, btd, bd = x.to(dev), g.to(dev), bt.to(dev), b.to(dev)
    wpk, s = ops.pack_conv_weight_f16s(w.to(dev))
    for groups, slope, act, og in ((8, -1.0, "gelu", 8), (C, 0.01, "lrelu", Cout)):
        ws = group_sums(x, groups).to(dev)
        coef = ops.group_norm_coef(ws, gd, btd, groups, B, C, H * W)
        with stream_forced(2):
            assert ops.prenorm_ok(xd, Cout)
            with launch_counts() as n:
                out, st = ops.conv2d_f16s_prenorm(xd, coef, slope, wpk, s, bd, Cout, stats_groups=og)
            assert n == {PK_STREAM: 1, PK_F16S: 0, PK_WINO: 0}, ("conv_stream did not take the layer", n)
            again = ops.conv2d_f16s_prenorm(xd, coef, slope, wpk, s, bd, Cout)
        with stream_forced(0):
            assert ops.prenorm_ok(xd, Cout)
            with launch_counts() as n:
                ref_out = ops.conv2d_f16s_prenorm(xd, coef, slope, wpk, s, bd, Cout)
            assert n == {PK_STREAM: 0, PK_F16S: 1, PK_WINO: 0}, n
        assert torch.equal(again, out), "repeat run differs"
        assert float((out - ref_out).abs().max()) <= 4e-6 * (1.0 + float(ref_out.abs().max()))
        a64 = TORCH_ACT[act](F.group_norm(x[sm].double(), groups, g.double(), bt.double(), eps=1e-5))
        want = F.conv2d(a64, w.double(), b.double(), padding=1)
        d = float((out[sm].cpu().double() - want).abs().max())
        print("\nconv_stream PRE %s %s: max|out - fp64| = %.2e (bar 2e-5), max|y| = %.1f" % (srow_id(row), act, d, float(want.abs().max())), end="")
        assert d <= 2e-5, (act, d)
        check_stats(out[sm].cpu(), st, B, og, sm)


# ------------------------------------------------------------------------------------------------------------------ declines
def fp64_conv(x1, x2, w, b):
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    return F.conv2d(xin.double(), w.double(), b.double(), padding=1)


@pytest.mark.parametrize("name,B,C,H,W,Cout,view", [
    ("w48", 2, 64, 16, 48, 128, False),          # W = 48 is no multiple of the 32-column tile
    ("h10", 2, 64, 10, 32, 128, False),          # H = 10 is no multiple of the smallest tile's 4 rows
    ("view", 2, 64, 16, 32, 128, True),          # a Winograd shape whose input sits 4 bytes off a 16-byte boundary
    ("view_c480", 2, 48, 16, 16, 480, True),
])
def test_conv2d_module_leaves_winograd_where_it_must(dev, name, B, C, H, W, Cout, view):
    """the Conv2d module sends what the Winograd kernel cannot take to conv_f16s (one launch of that family, none of the others) and still
    meets the fp64 contract; the misaligned input is fenced by NaNs"""
    from cineflow import ops
    from cineflow.nn import Conv2d
    x = randn(B, C, H, W, seed=40)
    w = randn(Cout, C, 3, 3, seed=41) / math.sqrt(C * 9)
    b = randn(Cout, seed=42)
    m = Conv2d(C, Cout, 3, padding=1)
    m.load_state_dict({"weight": w, "bias": b}, dev)
    xd = device_input(x, dev, view)
    with wino_forced(1):
        assert ops.wino_ok(B, C, 0, H, W, Cout) == view          # the shape query knows nothing of the pointer: the module checks it
        with launch_counts() as n:
            out, st = m(xd, stats_groups=8)
        assert n == {PK_F16S: 1, PK_WINO: 0, PK_STREAM: 0}, n
    ref = split_reference(x, w, b, m._ws, lambda a, k: F.conv2d(a, k, padding=1))
    o = out.cpu().double()
    assert ratio(o, ref["y3"], SPLIT_BAR * ref["A"]) <= 1.0
    assert float((o - ref["true"]).abs().max()) <= 1e-5
    check_stats(out.cpu(), st, B, 8, list(range(B)))
    if view:                                                         # and the library refuses the misaligned pointer when asked directly
        from cineflow._lib import CineflowError
        wpk, s = ops.pack_conv_weight_wino(w.to(dev))
        with pytest.raises(CineflowError):
            ops.conv2d_wino(xd, wpk, s, b.to(dev), Cout)


@pytest.mark.parametrize("name,B,C1,C2,H,W,Cout,kw", [
    ("odd_chunks", 8, 48, 0, 256, 256, 32, {}),                  # 3 chunks
    ("odd_chunks_cat", 8, 20, 8, 256, 256, 32, {}),              # 2 + 1 chunks
    ("few_tiles", 7, 32, 0, 256, 256, 32, {}),                   # 896 tiles < 1024
    ("few_tiles_64", 3, 64, 0, 256, 256, 64, {}),                # 768 tiles
    ("w_mod4", 8, 32, 0, 256, 254, 32, {}),                      # W % 4 != 0
    ("act", 8, 32, 0, 256, 256, 32, {"act": "relu"}),
    ("res", 4, 64, 0, 256, 256, 64, {"res": True}),
    ("slice", 8, 32, 0, 256, 256, 32, {"slice": True}),
    ("view", 8, 32, 0, 256, 256, 32, {"view": True}),            # misaligned input
    ("cout128", 8, 32, 0, 128, 128, 128, {}),                    # only 32 and 64 output channels
])
def test_conv_stream_declines(dev, name, B, C1, C2, H, W, Cout, kw):
    """layers outside conv_stream_applicable stay on conv_f16s_kernel at route level 2: the launch counters say so, and the result equals
    the level 0 result bit for bit, since the same kernel ran"""
    from cineflow import ops
    x1 = randn(B, C1, H, W, seed=50)
    x2 = randn(B, C2, H, W, seed=51).to(dev) if C2 else None
    w = randn(Cout, C1 + C2, 3, 3, seed=52) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=53).to(dev)
    x1d = device_input(x1, dev, bool(kw.get("view")))
    wpk, s = ops.pack_conv_weight_f16s(w.to(dev), c1=C1 if (C2 and C1 % 16) else None)
    res = randn(B, Cout, H, W, seed=54).to(dev) if kw.get("res") else None

    def run():
        big = torch.full((B, Cout + 5, H, W), 7.0, device=dev) if kw.get("slice") else None
        with launch_counts() as n:
            out = ops.conv2d_f16s(x1d, wpk, s, b, Cout, 3, 3, 1, (1, 1), x2=x2, act=kw.get("act"), res=res, out=big, out_coff=2 if big is not None else 0)
        return out, n

    with wino_forced(0):
        with stream_forced(2):
            got, n2 = run()
        with stream_forced(0):
            want, n0 = run()
    assert n2 == n0 == {PK_F16S: 1, PK_STREAM: 0, PK_WINO: 0}, (n2, n0)
    assert torch.equal(got, want)
    i = B - 1
    ref = fp64_conv(x1[i:i + 1], None if x2 is None else x2[i:i + 1].cpu(), w, b.cpu())
    if kw.get("act"):
        ref = TORCH_ACT[kw["act"]](ref)
    if res is not None:
        ref = ref + res[i:i + 1].cpu().double()
    o = got[i:i + 1, 2:2 + Cout] if kw.get("slice") else got[i:i + 1]
    assert float((o.cpu().double() - ref).abs().max()) <= 1e-5
    if kw.get("slice"):
        assert bool((got[:, :2] == 7.0).all()) and bool((got[:, 2 + Cout:] == 7.0).all())


def test_conv_stream_prenorm_declines(dev):
    """PRE outside the kernel: 64 output channels at the default level 1 (measured routing), an odd chunk count, too few tiles -- conv_f16s' PRE
    kernel runs and the result equals level 0 bit for bit"""
    from cineflow import ops
    for B, C, H, W, Cout, level in ((4, 64, 256, 256, 64, 1), (8, 48, 256, 256, 32, 2), (7, 32, 256, 256, 32, 2)):
        x, g, bt, w, b = prenorm_operands(B, C, H, W, Cout, 60 + B)
        xd = x.to(dev)
        wpk, s = ops.pack_conv_weight_f16s(w.to(dev))
        coef = ops.group_norm_coef(group_sums(x, 8).to(dev), g.to(dev), bt.to(dev), 8, B, C, H * W)
        outs = []
        for lv in (level, 0):
            with stream_forced(lv):
                assert ops.prenorm_ok(xd, Cout)
                with launch_counts() as n:
                    outs.append(ops.conv2d_f16s_prenorm(xd, coef, -1.0, wpk, s, b.to(dev), Cout))
                assert n == {PK_F16S: 1, PK_STREAM: 0, PK_WINO: 0}, (B, C, Cout, lv, n)
        assert torch.equal(outs[0], outs[1])
        i = B - 1
        a64 = F.gelu(F.group_norm(x[i:i + 1].double(), 8, g.double(), bt.double(), eps=1e-5))
        assert float((outs[0][i:i + 1].cpu().double() - F.conv2d(a64, w.double(), b.double(), padding=1)).abs().max()) <= 3e-5
