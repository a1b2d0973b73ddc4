"""conv_igemm_f32_kernel<1,2> and <2,2> (csrc/conv.hip), the exact fp32 route, held to the fmaf chain its header promises -- bit for bit.

entry point -> kernel -> rows
  cf_conv2d, Cout <= 32                  conv_igemm_f32_kernel<1,2>, counter PK_CONV_MT1 (0)   PLAIN_ROWS, EPI_ROWS[mt1], test_non_finite
  cf_conv2d, Cout > 32                   conv_igemm_f32_kernel<2,2>, counter PK_CONV_MT2 (1)   PLAIN_ROWS, EPI_ROWS[mt2]
  cf_conv2d, w_bstride != 0              either, weights per sample                            test_per_sample_weights
  cf_conv_transpose2d_k2s2               either on 4 Cout GEMM rows, scatter2x2 epilogue       CONVT_ROWS
  cf_corr_pyramid, W != 32               conv_igemm_f32_kernel<2,2>, counter PK_ALLPAIRS (7)   test_pyramid_level0
Every row reads the launch counters of cf_profile_read and fails if another instantiation (or none) took the launch.  The host-side argument
checks of cf_conv2d run without a device: tests/test_abi_and_host.py::test_conv2d_argument_checks_need_no_gpu.

Reference (tests/_fma_chain.py, held to libm's fmaf in test_fma_chain_cpu.py).  v_mfma_f32_32x32x2_f32 computes
D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) with one rounding per product; lanes 0-31 carry k, lanes 32-63 k + 1; the kernel walks
k = ci KH KW + kh KW + kw from 0 in steps of two from accumulators of +0 and feeds zeros for padding taps and for k >= K.  So the plain
output (no bias, alpha 1, no activation, no residual) must EQUAL y32 = the fp32 fmaf chain in that order: no tolerance, no element
excluded, compared with torch.equal after printing the mismatch count.  What the chain says about small numbers: nothing is flushed.  A
product or partial sum below 2^-126 is a subnormal with fewer bits and rounds once like any other (gradual underflow); the "tiny" row
(x 1e-25, w 1e-15: every output is subnormal, around 1e-39) asserts that the outputs are subnormal, non-zero and equal to the chain, so a
kernel built with flushed denormals (A / B operands flushed to zero) fails it on every element.
The chain's k order matters: reversed, or with the two k of one MFMA swapped, 65 - 87 % of the elements of a 3x3 16-channel row change
(test_fma_chain_cpu.py), all inside every tolerance the suite had.

Other bars.
  older contract       max|out - y64| <= 2e-5 on every finite row with unit operands (x ~ N(0,1), w ~ N(0,1) / sqrt(K)), the figure of
                       test_gpu_ops.py::test_conv2d; on the three amplitude rows 2e-5 x max(1, max|y64|), the form the Winograd table gives
                       the same contract (an absolute 2e-5 is below one ulp of outputs near 2000).
  epilogue             fp64 act(alpha acc + b) + res, acc = the plain output of the same operands from the same kernel, at
                       2e-6 (1 + |pre| + |res|), pre = alpha acc + b: the Winograd table's bar for the same formula.
  bias only            alpha = 1, no activation: bit-equal to fl32(y32 + b) (fma(1, acc, b) and fl(fl(1 acc) + b) are the same number, so the
                       contraction the compiler chooses for alpha * acc + b cannot show).
  res is out           dense destination: bit-equal to the out-of-place call (the composed Conv3d's depth-tap accumulate).
  transposed           bit-equal to fl32(chain + b[co]) at out[b, co, 2 y + dy, 2 x + dx], GEMM row m = co 4 + dy 2 + dx, k = ci.
  per-sample weights   each sample bit-equal to the chain of its own weights.
  pyramid level 0      bit-equal to fl32(fl32(1 / sqrt(C)) chain), chain over c of f1[b, c, n1] f2[b, c, n2].
  non-finite           elements whose receptive field holds neither planted value: bit-equal to the chain; the others carry the NaN mask and
                       the Inf signs of F.conv2d in fp64.  The excluded share comes from the reference alone (6.1 %).

What the plain rows reach (B, C1 + C2, H x W, Cout, kernel, stride, pad); Cout x pixels x K <= 5e7 on every row:
  Cout blocks   1, 5, 32 (last MT1), 33 (first MT2), 64, 65, 70 (two grid.y blocks, the second ragged) at 1 x 3 x 9 x 11, 3x3: K = 27 odd
  pixel tiles   35 pixels (< 64); 322 = 256 + 66 (waves 2 and 3 of the last workgroup exit, wave 1 holds two pixels); 3 samples of 99 pixels
                (a wave tile spans two samples); 1 x 52 x 54 = 2808 pixels = 11 tiles (xcd_band_remap with q = 1, r = 3) at Cout 64 (one
                channel block) and 70 (two); every other row has fewer than 8 tiles (q = 0)
  K             1; 2, 5, 7 (< 8 = 2 PF: the prologue alone passes K); 8, 9, 10 (one loop trip, slots refilled past K); 16, 17; 9 as 1 channel 3x3;
                864 (96 channels 3x3 on 8 x 8, Cout 160)
  k cursor      KW = 1 with KH = 1, 2, 3, 5 (kw wraps twice per step); KH = 1 with KW = 2, 5; 2x2; 7x7 on 2 channels to 128 (the motion
                encoder); 15x15 pad 7; 1x15 pad (0, 7)
  stride, pad   strides 1 - 4 on 13 x 17; 4x4 stride 4 pad 0; 3x3 pad 0, (0, 2), (2, 0); 3x3 pad 3 (whole output rows of padding: exact 0)
  dual input    C1 = 1 and 3 at 3x3 (C1 KH KW odd: one two-k step takes a k from each input); 8 + 8; C2 = 1
  views         x1, x2 and out one float off a 16-byte boundary, inputs fenced by NaN, output by a sentinel that must survive
  amplitudes    x 1e5, w 1e-3; x 1e-25, w 1e-15 (subnormal outputs); both per channel (x channels alternate 1e5 / 1e-25, output channels'
                weights 1e-3 / 1e-15: products of 1e2, 1e-10, 1e-28 and 1e-40 in the same launch)

Measured on the MI355X (pytest -s prints one line per row; every line is in profiles/conv_f32_route_table.md): 0 of 929,741 elements of
the plain, transposed, per-sample-weight and pyramid rows differ from the chain, the subnormal rows included; max|out - y64| is 1.8e-7 -
1.5e-6 on the unit rows with K <= 450 and 3.7e-6 at K = 864; the epilogue rows sit at 0.027 - 0.062 of their bar (GELU the largest);
tools/kernel_coverage.py on a kernel trace of this file: <1,2> 47 dispatches, <2,2> 62.

Findings.
  None in the kernel: the header statement of csrc/conv.hip holds on every row as written, gradual underflow included, and the
  epilogue's alpha * acc + b equals fl32(acc + b) at alpha = 1 and fl32(alpha acc) at b = 0, whichever contraction the compiler chose.
  Two things this file had to settle for itself:
  1. The older contract is an absolute 2e-5 for outputs of unit scale.  The "big" and "mixed" rows have outputs near 2000, where one ulp
     is 1.2e-4: they carry it relative to max|y64| (bars above).  The "tiny" rows meet the absolute figure trivially; what holds them
     is the bit comparison.
  2. A reference built on fl32(fl64(a b + c)) is not the chain: it rounds twice (tests/_fma_chain.py, DOUBLE_ROUNDING_TRIPLES).  None of
     60,000 random triples shows it, so such a reference would have passed a long time before failing one element of one row.

Mutations (scratch builds of csrc/conv.hip, every access kept inside its buffer; "old" = the 156 GPU tests around this kernel from before
this file: test_gpu_ops.py -k conv, the all-pairs pyramids of test_gpu_flow_op_shapes.py, test_gpu_module_routes.py):
  1. half-waves swapped (lk = 1 - half, kw = 1 - half: each pair of products added in the other order)
                                      82 of the 100 tests here fail: every plain row with K >= 2 but the tiny ones (55 - 61 % of the
                                      elements of the Cout rows), non-finite, exact forms, 7 of 8 transposed, per-sample weights, pyramid.
                                      The tiny rows pass, and must: sums of subnormals are fixed-point additions on the 2^-149 grid and
                                      do not depend on the order.  old: 156 pass
  2. xcd_band_remap: r * q for r * (q + 1) in the second branch (wrong only with more than 8 tiles and a remainder)
                                      the three tiles11 rows fail (tiles 8 - 10 never written: NaN).  old: 156 pass
  3. conv.hip built with -fgpu-flush-denormals-to-zero
                                      tiny and tiny_mt1 fail on every element.  old: 156 pass
"""
import contextlib
import ctypes
import math
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _fma_chain import conv_chain_reference, convT_chain_reference
from _split_exact import ACTS, TORCH_ACT, device_input, randn

pytestmark = pytest.mark.gpu

PK_CONV_MT1, PK_CONV_MT2, PK_CONV_MT4, PK_ALLPAIRS = 0, 1, 2, 7
SENT = -12345.5
NAN = float("nan")
BUDGET = 5e7                                           # Cout x pixels x K of one row: about a second of CPU chain


@contextlib.contextmanager
def launch_counts():
    """{kernel id: launches} of the fp32 implicit-GEMM family and the all-pairs volume for the calls made inside (filled on exit)"""
    from cineflow._lib import check, lib
    h = lib()
    got = {}
    check(h.cf_profile_enable(64), "cf_profile_enable")
    try:
        yield got
        torch.cuda.synchronize()
        for kid in (PK_CONV_MT1, PK_CONV_MT2, PK_CONV_MT4, PK_ALLPAIRS):
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
            check(h.cf_profile_read(kid, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)), "cf_profile_read")
            got[kid] = n.value
    finally:
        check(h.cf_profile_enable(0), "cf_profile_enable")


def expected_counts(cout_rows, n=1):
    """the launches a call with `cout_rows` GEMM rows must book: launch_conv picks MT = 1 up to 32 rows, MT = 2 beyond"""
    return {PK_CONV_MT1: n if cout_rows <= 32 else 0, PK_CONV_MT2: n if cout_rows > 32 else 0, PK_CONV_MT4: 0, PK_ALLPAIRS: 0}


def mismatches(got, want):
    """elements that differ (NaN on both sides counts as equal; -0 equals +0)"""
    return int(((got != want) & ~(torch.isnan(got) & torch.isnan(want))).sum())


def fenced_out(dev, shape, view):
    """a NaN-filled output (an element no wave wrote stays NaN); view=True: one float into a buffer of sentinels -> (out, check)"""
    n = int(np.prod(shape))
    if not view:
        return torch.full(shape, NAN, device=dev), lambda: None
    buf = torch.full((n + 8,), SENT, device=dev)
    out = buf[1:1 + n].view(shape)
    out.fill_(NAN)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4

    def check():
        host = buf.cpu()
        assert float(host[0]) == SENT and bool((host[1 + n:] == SENT).all()), "the kernel wrote outside its output"
    return out, check


# ================================================================================================================== plain rows
Row = namedtuple("Row", "name B C1 C2 H W Cout KH KW stride pad amp view", defaults=(None, False))
SMALL = (1, 3, 0, 9, 11)                               # B, C1, C2, H, W of the Cout rows: 99 pixels, K = 27
PLAIN_ROWS = (
    # ---- Cout blocks
    [Row("cout%d" % c, *SMALL, c, 3, 3, 1, (1, 1)) for c in (1, 5, 32, 33, 64, 65, 70)]
    + [
        # ---- pixel tiles
        Row("pix35", 1, 3, 0, 5, 7, 5, 3, 3, 1, (1, 1)),
        Row("pix322_mt1", 1, 3, 0, 14, 23, 5, 3, 3, 1, (1, 1)),
        Row("pix322_mt2", 1, 3, 0, 14, 23, 40, 3, 3, 1, (1, 1)),
        Row("samples3_mt1", 3, 3, 0, 9, 11, 20, 3, 3, 1, (1, 1)),
        Row("samples3_mt2", 3, 3, 0, 9, 11, 70, 3, 3, 1, (1, 1)),
        Row("tiles11_y1", 1, 3, 0, 52, 54, 64, 3, 3, 1, (1, 1)),
        Row("tiles11_y2", 1, 3, 0, 52, 54, 70, 3, 3, 1, (1, 1)),
        Row("tiles11_mt1", 1, 3, 0, 52, 54, 7, 3, 3, 1, (1, 1)),
    ]
    # ---- K around the prefetch depth (1x1: K = Cin), both instantiations
    + [Row("k%d_c%d" % (k, c), 2, k, 0, 7, 9, c, 1, 1, 1, (0, 0)) for k in (1, 2, 5, 7, 8, 9, 10, 16, 17) for c in (5, 33)]
    + [
        Row("k9_3x3", 2, 1, 0, 7, 9, 33, 3, 3, 1, (1, 1)),
        Row("k864", 1, 96, 0, 8, 8, 160, 3, 3, 1, (1, 1)),
        # ---- k cursor
        Row("kh1_kw1", 1, 3, 0, 9, 11, 33, 1, 1, 1, (0, 0)),
        Row("kh2_kw1", 1, 3, 0, 9, 11, 33, 2, 1, 1, (1, 0)),
        Row("kh3_kw1", 1, 3, 0, 9, 11, 33, 3, 1, 1, (1, 0)),
        Row("kh5_kw1", 1, 3, 0, 9, 11, 5, 5, 1, 1, (2, 0)),
        Row("kh1_kw2", 1, 3, 0, 9, 11, 33, 1, 2, 1, (0, 1)),
        Row("kh1_kw5", 1, 3, 0, 9, 11, 5, 1, 5, 1, (0, 2)),
        Row("k2x2", 1, 3, 0, 9, 11, 33, 2, 2, 1, (0, 0)),
        Row("motion7x7", 1, 2, 0, 16, 16, 128, 7, 7, 1, (3, 3)),
        Row("k15x15", 1, 2, 0, 9, 10, 5, 15, 15, 1, (7, 7)),
        Row("k15x15_mt2", 1, 1, 0, 9, 10, 33, 15, 15, 1, (7, 7)),
        Row("k1x15", 1, 3, 0, 5, 20, 33, 1, 15, 1, (0, 7)),
    ]
    # ---- stride and pad
    + [Row("stride%d_c%d" % (s, c), 2, 3, 0, 13, 17, c, 3, 3, s, (1, 1)) for s in (1, 2, 3, 4) for c in (5, 33)]
    + [
        Row("patch4x4_s4", 2, 3, 0, 13, 17, 33, 4, 4, 4, (0, 0)),
        Row("s3_5x5", 1, 2, 0, 13, 17, 5, 5, 5, 3, (2, 2)),
        Row("pad0", 1, 3, 0, 9, 11, 33, 3, 3, 1, (0, 0)),
        Row("pad0_2", 1, 3, 0, 9, 11, 5, 3, 3, 1, (0, 2)),
        Row("pad2_0", 1, 3, 0, 9, 11, 33, 3, 3, 1, (2, 0)),
        Row("pad3_3x3", 1, 3, 0, 9, 11, 33, 3, 3, 1, (3, 3)),
        Row("pad3_3x3_s2", 1, 3, 0, 9, 11, 5, 3, 3, 2, (3, 3)),
        # ---- dual input
        Row("cat1_4", 2, 1, 4, 9, 11, 33, 3, 3, 1, (1, 1)),
        Row("cat3_2", 2, 3, 2, 9, 11, 5, 3, 3, 1, (1, 1)),
        Row("cat8_8", 1, 8, 8, 9, 11, 33, 3, 3, 1, (1, 1)),
        Row("cat5_1", 1, 5, 1, 9, 11, 33, 3, 3, 2, (1, 1)),
        Row("cat3_1_1x1", 1, 3, 1, 9, 11, 5, 1, 1, 1, (0, 0)),
        # ---- views
        Row("views_mt1", 2, 3, 2, 9, 11, 20, 3, 3, 1, (1, 1), None, True),
        Row("views_mt2", 2, 3, 2, 9, 11, 70, 3, 3, 1, (1, 1), None, True),
        # ---- dynamic range
        Row("big", 2, 3, 0, 9, 11, 33, 3, 3, 1, (1, 1), (1e5, 1e-3)),
        Row("tiny", 2, 3, 0, 9, 11, 33, 3, 3, 1, (1, 1), (1e-25, 1e-15)),
        Row("tiny_mt1", 2, 3, 0, 9, 11, 5, 3, 3, 1, (1, 1), (1e-25, 1e-15)),
        Row("mixed", 2, 6, 0, 9, 11, 34, 3, 3, 1, (1, 1), "mixed"),
    ]
)
assert len({r.name for r in PLAIN_ROWS}) == len(PLAIN_ROWS)


def geometry(r):
    Ho, Wo = (r.H + 2 * r.pad[0] - r.KH) // r.stride + 1, (r.W + 2 * r.pad[1] - r.KW) // r.stride + 1
    return Ho, Wo, (r.C1 + r.C2) * r.KH * r.KW


def operands(r, seed):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(K) (outputs of unit scale), then the row's amplitudes"""
    K = geometry(r)[2]
    x1 = randn(r.B, r.C1, r.H, r.W, seed=seed)
    x2 = randn(r.B, r.C2, r.H, r.W, seed=seed + 1) if r.C2 else None
    w = randn(r.Cout, r.C1 + r.C2, r.KH, r.KW, seed=seed + 2) / math.sqrt(K)
    if r.amp == "mixed":
        assert r.C2 == 0
        x1 = x1 * torch.tensor([1e5, 1e-25] * (r.C1 // 2)).view(1, -1, 1, 1)
        w = w * math.sqrt(K) * torch.tensor([1e-3, 1e-15] * (r.Cout // 2)).view(-1, 1, 1, 1)
    elif r.amp is not None:
        x1, w = x1 * r.amp[0], w * math.sqrt(K) * r.amp[1]
        x2 = None if x2 is None else x2 * r.amp[0]
    return x1, x2, w


def run_conv(dev, r, x1, x2, w, **kw):
    """ops.conv2d into a NaN-filled (and, on view rows, fenced) output -> CPU tensor; asserts the launch counter"""
    from cineflow import ops
    Ho, Wo, K = geometry(r)
    x1d = device_input(x1, dev, r.view)
    x2d = None if x2 is None else device_input(x2, dev, r.view)
    out, fence = fenced_out(dev, (r.B, r.Cout, Ho, Wo), r.view)
    with launch_counts() as n:
        ops.conv2d(x1d, ops.prep_conv_weight(w).to(dev), kw.pop("bias", None), r.Cout, r.KH, r.KW, r.stride, r.pad, x2=x2d, out=out, **kw)
    assert n == expected_counts(r.Cout), "%s: launches %s, expected %s" % (r.name, n, expected_counts(r.Cout))
    fence()
    assert torch.equal(x1d.cpu().view(torch.int32), x1.view(torch.int32)), "x1 changed"
    return out.cpu()


@pytest.mark.parametrize("r", PLAIN_ROWS, ids=[r.name for r in PLAIN_ROWS])
def test_plain_rows(dev, r):
    Ho, Wo, K = geometry(r)
    npix = r.B * Ho * Wo
    assert r.Cout * npix * K <= BUDGET
    ntiles = -(-npix // 256)
    if r.name.startswith("tiles11"):
        assert ntiles == 11 and -(-r.Cout // (32 if r.Cout <= 32 else 64)) == (2 if r.name.endswith("y2") else 1)
    else:
        assert ntiles < 8
    if r.name.startswith("samples3"):
        assert r.B > 1 and (Ho * Wo) % 64 != 0
    x1, x2, w = operands(r, 5000 + 10 * PLAIN_ROWS.index(r))
    y32, y64, A = conv_chain_reference(x1, x2, w, r.stride, r.pad)
    got = run_conv(dev, r, x1, x2, w)
    bad = mismatches(got, y32)
    d = float((got.double() - y64).abs().max())
    scale = 1.0 if r.amp is None else max(1.0, float(y64.abs().max()))
    print("\n%-14s %d x (%d + %d) x %d x %d -> %d, %d x %d / %d pad %s: <%d,2>, K = %d, %d pixels, %d of %d elements differ from the chain, "
          "max|out - y64| = %.2e (bar %.1e)" % (r.name, r.B, r.C1, r.C2, r.H, r.W, r.Cout, r.KH, r.KW, r.stride, r.pad, 1 if r.Cout <= 32 else 2,
                                                K, npix, bad, got.numel(), d, 2e-5 * scale))
    assert bool(torch.isfinite(y32).all())
    if r.name.startswith("pad3"):
        assert bool((y32[:, :, 0] == 0).all()) and bool((got[:, :, 0] == 0).all()), "an output row of padding only is not 0"
    if r.name.startswith("tiny"):
        sub = (y32.abs() < 2.0 ** -126) & (y32 != 0)
        assert bool(sub.all()), "the row is meant to produce subnormal outputs only"
    if r.amp == "mixed":
        assert float(y32[:, 0::2].abs().max()) > 1e2 and 0 < float(y32[:, 1::2].abs().max()) < 1e-8
    assert bad == 0 and torch.equal(got, y32), "%s: %d of %d elements differ from the fmaf chain" % (r.name, bad, got.numel())
    assert d <= 2e-5 * scale, "%s: older contract, max|out - y64| = %.3e" % (r.name, d)


# ================================================================================================================== non-finite
def test_non_finite(dev):
    """3 x 4 x 9 x 11 -> 20, 3x3: a NaN at x[0, 1, 2, 3] and a +Inf at x[0, 2, 6, 8].  The excluded set is where the fp64 reference is
    not finite (2 x 9 pixels of sample 0, every channel: 6.1 % of the output)."""
    r = Row("nonfinite", 3, 4, 0, 9, 11, 20, 3, 3, 1, (1, 1))
    x1, _, w = operands(r, 6100)
    x1[0, 1, 2, 3] = NAN
    x1[0, 2, 6, 8] = float("inf")
    true = F.conv2d(x1.double(), w.double(), padding=1)
    touched = ~torch.isfinite(true)
    share = float(touched.double().mean())
    assert 0 < share < 0.10 and int(touched[0, 0].sum()) == 18 and not bool(touched[1:].any())
    assert int(torch.isnan(true).sum()) == 9 * r.Cout and int(torch.isinf(true).sum()) == 9 * r.Cout
    y32, _, _ = conv_chain_reference(x1, None, w, 1, (1, 1))
    got = run_conv(dev, r, x1, None, w)
    bad = int((got[~touched] != y32[~touched]).sum())
    print("\nnon-finite: %.1f %% excluded, %d of %d other elements differ from the chain" % (100 * share, bad, int((~touched).sum())))
    assert bad == 0 and bool(torch.isfinite(got[~touched]).all())
    assert torch.equal(torch.isnan(got), torch.isnan(true)), "NaN mask differs from F.conv2d in fp64"
    inf = torch.isinf(true)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(torch.sign(got[inf]).double(), torch.sign(true[inf])), "Inf set or signs differ"
    assert bool((torch.sign(true[inf]) > 0).any()) and bool((torch.sign(true[inf]) < 0).any())
    d = float((got.double() - true)[~touched].abs().max())
    assert d <= 2e-5, d


# ================================================================================================================== epilogue
EPI_ROWS = {"mt1": Row("epi_mt1", 2, 3, 2, 9, 11, 20, 3, 3, 1, (1, 1)), "mt2": Row("epi_mt2", 2, 3, 2, 13, 11, 40, 3, 3, 2, (1, 1))}
_EPI = {}


def epi_case(dev, key):
    """operands, bias, residual and the same kernel's plain output of an epilogue geometry, made once and left unchanged"""
    if key not in _EPI:
        r = EPI_ROWS[key]
        x1, x2, w = operands(r, 6200 + (key == "mt2"))
        Ho, Wo, K = geometry(r)
        c = dict(r=r, x1=x1, x2=x2, w=w, b=randn(r.Cout, seed=6210), res=randn(r.B, r.Cout, Ho, Wo, seed=6211))
        c["plain"] = run_conv(dev, r, x1, x2, w)
        _EPI[key] = c
    return _EPI[key]


@pytest.mark.parametrize("act", (None,) + ACTS)
@pytest.mark.parametrize("key", ["mt1", "mt2"])
def test_epilogue(dev, key, act):
    """act(0.75 acc + b) + res into channels [2, 2 + Cout) of a sentinel-filled tensor, against fp64 on the same launch's plain output"""
    from cineflow import ops
    c = epi_case(dev, key)
    r, plain = c["r"], c["plain"]
    Ho, Wo, K = geometry(r)
    big = torch.full((r.B, r.Cout + 5, Ho, Wo), SENT, device=dev)
    with launch_counts() as n:
        ops.conv2d(c["x1"].to(dev), ops.prep_conv_weight(c["w"]).to(dev), c["b"].to(dev), r.Cout, r.KH, r.KW, r.stride, r.pad, x2=c["x2"].to(dev),
                   act=act, res=c["res"].to(dev), out=big, out_coff=2, alpha=0.75)
    assert n == expected_counts(r.Cout), n
    host = big.cpu()
    assert bool((host[:, :2] == SENT).all()) and bool((host[:, 2 + r.Cout:] == SENT).all()), "sentinel channels written"
    pre = 0.75 * plain.double() + c["b"].double().view(1, -1, 1, 1)
    rs = c["res"].double()
    want = (pre if act is None else TORCH_ACT[act](pre)) + rs
    ratio = float(((host[:, 2:2 + r.Cout].double() - want).abs() / (2e-6 * (1.0 + pre.abs() + rs.abs()))).max())
    print("\nepilogue %s %-7s <%d,2>: worst |out - fp64| / (2e-6 (1 + |pre| + |res|)) = %.4f" % (key, act, 1 if r.Cout <= 32 else 2, ratio))
    assert ratio <= 1.0, (key, act, ratio)


@pytest.mark.parametrize("key", ["mt1", "mt2"])
def test_epilogue_exact_forms(dev, key):
    """the plain output is the chain; alpha = 1 with a bias and no activation is fl32(y32 + b); res is out is the out-of-place call"""
    from cineflow import ops
    c = epi_case(dev, key)
    r = c["r"]
    y32, y64, _ = conv_chain_reference(c["x1"], c["x2"], c["w"], r.stride, r.pad)
    assert torch.equal(c["plain"], y32), "%d elements of the plain output differ from the chain" % mismatches(c["plain"], y32)
    assert float((c["plain"].double() - y64).abs().max()) <= 2e-5
    biased = run_conv(dev, r, c["x1"], c["x2"], c["w"], bias=c["b"].to(dev))
    want = y32 + c["b"].view(1, -1, 1, 1)              # one fp32 addition per element
    assert want.dtype == torch.float32
    bad = mismatches(biased, want)
    print("\n%s: bias only, %d of %d elements differ from fl32(y32 + b)" % (key, bad, want.numel()))
    assert bad == 0
    x1d, x2d, wt, bd = c["x1"].to(dev), c["x2"].to(dev), ops.prep_conv_weight(c["w"]).to(dev), c["b"].to(dev)
    for act in (None, "gelu"):
        apart = ops.conv2d(x1d, wt, bd, r.Cout, r.KH, r.KW, r.stride, r.pad, x2=x2d, act=act, res=c["res"].to(dev), alpha=0.75)
        acc = c["res"].to(dev).clone()
        with launch_counts() as n:
            ops.conv2d(x1d, wt, bd, r.Cout, r.KH, r.KW, r.stride, r.pad, x2=x2d, act=act, res=acc, out=acc, alpha=0.75)
        assert n == expected_counts(r.Cout), n
        bad = mismatches(acc.cpu(), apart.cpu())
        print("%s: res is out (%s), %d of %d elements differ from the out-of-place call" % (key, act, bad, acc.numel()))
        assert bad == 0


# ================================================================================================================== transposed
CONVT_ROWS = [   # B, Cin, H, W, Cout, bias, slice
    (2, 20, 5, 7, 8, True, False),                     # 32 GEMM rows: the last MT1
    (1, 20, 5, 7, 8, False, True),
    (1, 20, 5, 7, 9, False, True),                     # 36: the first MT2
    (2, 6, 3, 5, 9, True, False),
    (3, 7, 3, 5, 16, True, True),                      # 64: one full block
    (2, 33, 9, 3, 17, False, False),                   # 68: two blocks, the second holds one output channel
    (2, 33, 9, 3, 17, True, True),
    (1, 1, 1, 1, 1, True, False),                      # one pixel, one k, four rows
]


@pytest.mark.parametrize("B,Cin,H,W,Cout,bias,sliced", CONVT_ROWS)
def test_transposed_rows(dev, B, Cin, H, W, Cout, bias, sliced):
    from cineflow import ops
    seed = 6300 + 7 * CONVT_ROWS.index((B, Cin, H, W, Cout, bias, sliced))
    x, w = randn(B, Cin, H, W, seed=seed), randn(Cin, Cout, 2, 2, seed=seed + 1) / math.sqrt(Cin)
    b = randn(Cout, seed=seed + 2) if bias else None
    y32, y64, _ = convT_chain_reference(x, w)
    want = y32 if b is None else y32 + b.view(1, -1, 1, 1)
    ctot, coff = (Cout + 5, 2) if sliced else (Cout, 0)
    big = torch.full((B, ctot, 2 * H, 2 * W), SENT if sliced else NAN, device=dev)
    if sliced:
        big[:, coff:coff + Cout] = NAN
    with launch_counts() as n:
        ops.conv_transpose2d_k2s2(x.to(dev), w.to(dev), None if b is None else b.to(dev), out=big, out_coff=coff)
    assert n == expected_counts(4 * Cout), n
    host = big.cpu()
    got = host[:, coff:coff + Cout]
    bad = mismatches(got, want)
    print("\nconvT %d x %d x %d x %d -> %d%s%s: <%d,2>, %d of %d elements differ from fl32(chain + b)" % (
        B, Cin, H, W, Cout, ", bias" if bias else "", ", slice" if sliced else "", 1 if 4 * Cout <= 32 else 2, bad, got.numel()))
    assert bad == 0
    if sliced:
        assert bool((host[:, :coff] == SENT).all()) and bool((host[:, coff + Cout:] == SENT).all()), "sentinel channels written"
    ref = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2)
    assert float((got.double() - ref).abs().max()) <= 2e-5


# ================================================================================================================== per-sample weights
@pytest.mark.parametrize("H,W,C,Cout,k", [(8, 8, 3, 33, 3), (8, 16, 5, 20, 1), (8, 16, 3, 70, 3)])
def test_per_sample_weights(dev, H, W, C, Cout, k):
    """w_bstride = K Cout through the ABI, B = 3: 64 pixels (one wave tile per sample, four samples' worth of waves in a workgroup) and 128"""
    from cineflow import ops
    B, K, pad = 3, C * k * k, (k // 2, k // 2)
    x = randn(B, C, H, W, seed=6400 + W + k)
    w = randn(B, Cout, C, k, k, seed=6401 + W + k) / math.sqrt(K)
    wt = torch.stack([ops.prep_conv_weight(w[b]) for b in range(B)]).contiguous()
    assert wt.shape == (B, K, Cout)
    out = torch.full((B, Cout, H, W), NAN, device=dev)
    with launch_counts() as n:
        ops.conv2d(x.to(dev), wt.to(dev), None, Cout, k, k, 1, pad, out=out, w_bstride=K * Cout)
    assert n == expected_counts(Cout), n
    got = out.cpu()
    for b in range(B):
        y32, y64, _ = conv_chain_reference(x[b:b + 1], None, w[b], 1, pad)
        bad = mismatches(got[b:b + 1], y32)
        print("\nper-sample weights %d x %d, sample %d: %d of %d elements differ from the chain of its own weights" % (H, W, b, bad, y32.numel()))
        assert bad == 0
        assert float((got[b:b + 1].double() - y64).abs().max()) <= 2e-5
        if b:
            assert mismatches(got[b:b + 1], conv_chain_reference(x[b:b + 1], None, w[0], 1, pad)[0]) > 0      # the weights do differ


def test_per_sample_weights_need_whole_wave_tiles(dev):
    from cineflow import ops
    from cineflow._lib import CineflowError
    x, wt = torch.zeros(3, 3, 8, 8, device=dev), torch.zeros(3, 27, 5, device=dev)
    with pytest.raises(CineflowError, match=r"per-sample weights need Ho\*Wo % 64 == 0 \(got 16\)"):
        ops.conv2d(x, wt, None, 5, 3, 3, 2, (1, 1), w_bstride=27 * 5)
    with pytest.raises(CineflowError, match=r"per-sample weights need Ho\*Wo % 64 == 0 \(got 36\)"):
        ops.conv2d(x, wt, None, 5, 3, 3, 1, (0, 0), w_bstride=27 * 5)


def test_pyramid_level0(dev):
    """cf_corr_pyramid at 2 x 32 x 16 x 20 (a test_raft_maps row: W = 20, the fused kernel declines): level 0 is the per-sample-weight GEMM
    with alpha = fl32(1 / sqrt(C)), out[b, n1, n2] = fl32(alpha x chain over c of f1[b, c, n1] f2[b, c, n2]); 320 GEMM rows: <2,2>"""
    from cineflow import ops
    B, C, H, W, levels = 2, 32, 16, 20, 4
    N = H * W
    assert N % 64 == 0 and N * N * C <= BUDGET
    f1, f2 = randn(B, C, H, W, seed=6500), randn(B, C, H, W, seed=6501)
    with launch_counts() as n:
        pyr = ops.corr_pyramid(f1.to(dev), f2.to(dev), levels)
    assert n == {PK_CONV_MT1: 0, PK_CONV_MT2: 0, PK_CONV_MT4: 0, PK_ALLPAIRS: levels}, n      # the GEMM and three pooling launches
    got = pyr[:B * N * N].view(B, N, H, W).cpu()
    alpha = torch.tensor(1.0 / math.sqrt(float(C)), dtype=torch.float64).float()
    for b in range(B):
        y32, y64, _ = conv_chain_reference(f2[b:b + 1], None, f1[b].reshape(C, N).t().reshape(N, C, 1, 1), 1, (0, 0))
        want = alpha * y32                              # one fp32 product per element
        assert want.dtype == torch.float32
        bad = mismatches(got[b:b + 1], want)
        print("\npyramid level 0, sample %d: %d of %d elements differ from fl32(fl32(1 / sqrt(C)) x chain)" % (b, bad, want.numel()))
        assert bad == 0
        assert float((got[b:b + 1].double() - y64 / math.sqrt(C)).abs().max()) <= 2e-5
