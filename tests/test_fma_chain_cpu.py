"""tests/_fma_chain.py on the CPU: fma32 is libm's fmaf, a plain fp64 evaluation is not, the convolution chain obeys its deterministic bound,
and the chain depends on its k order -- so a kernel with another order cannot equal it by accident.  The chain that starts from a bias
(direct_conv_reference, the direct small-channel kernels) is a scalar loop over fmaf too, and is not the chain from +0 plus the bias."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _fma_chain import DOUBLE_ROUNDING_TRIPLES, conv_chain_reference, convT_chain_reference, direct_conv_reference, fma32, fma32_plain

U = 2.0 ** -24                                         # unit roundoff of fp32


@pytest.fixture(scope="module")
def fmaf():
    path = ctypes.util.find_library("m") or "libm.so.6"
    fn = ctypes.CDLL(path).fmaf
    fn.argtypes = [ctypes.c_float] * 3
    fn.restype = ctypes.c_float

    def many(a, b, c):
        return np.array([fn(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    return many


def same_bits(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    return (got.view(np.uint32) == want.view(np.uint32)) | both_nan


def test_fma32_is_fmaf_on_random_triples(fmaf):
    """60 000 triples: c = +-|a b| x 10^e with e uniform in [-8, 8] (16 decades: from c lost below the product's last bit to the product lost
    below c's), a tenth of them with c within a few ulp of -a b (cancellation), a tenth scaled into the fp32 subnormal range"""
    rng = np.random.default_rng(20240)
    n = 60000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    c = (np.abs(p) * 10.0 ** rng.uniform(-8, 8, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    near = slice(0, n // 10)
    c[near] = (-p[near] * (1.0 + rng.integers(-4, 5, n // 10) * 2.0 ** -23)).astype(np.float32)
    tiny = slice(n // 10, n // 5)
    a[tiny] *= np.float32(1e-20)
    b[tiny] *= np.float32(1e-20)
    c[tiny] *= np.float32(1e-40)
    want = fmaf(a, b, c)
    assert int((np.abs(want[tiny]) < 2.0 ** -126).sum()) > n // 20, "the subnormal tenth is not subnormal"
    assert int((want[tiny] != 0).sum()) > n // 20, "the subnormal tenth underflowed to zero"
    ok = same_bits(fma32(a, b, c), want)
    assert ok.all(), "%d of %d triples differ from fmaf, first (%r, %r, %r)" % ((~ok).sum(), n, *[v[~ok][0] for v in (a, b, c)])
    plain = same_bits(fma32_plain(a, b, c), want)
    print("\nplain fl32(fl64(a b + c)) differs from fmaf on %d of %d random triples" % (int((~plain).sum()), n))


def test_fma32_is_fmaf_where_a_plain_cast_rounds_twice(fmaf):
    a, b, c = DOUBLE_ROUNDING_TRIPLES.T.copy()
    assert len(a) == 12
    assert ((a.astype(np.float64) * b.astype(np.float64)).astype(np.float32).astype(np.float64) != a.astype(np.float64) * b.astype(np.float64)).all()
    want = fmaf(a, b, c)
    assert same_bits(fma32(a, b, c), want).all()
    assert not same_bits(fma32_plain(a, b, c), want).any(), "the plain cast is right on a constructed triple: the helper would not be needed"
    # the benign direction (c points at the even neighbour): both agree with fmaf
    want = fmaf(a, b, -c)
    assert same_bits(fma32(a, b, -c), want).all() and same_bits(fma32_plain(a, b, -c), want).all()


def test_fma32_special_values(fmaf):
    inf, nan = float("inf"), float("nan")
    rows = np.array([(inf, 1.0, 1.0), (inf, 0.0, 1.0), (1.0, 1.0, nan), (inf, 1.0, -inf), (-inf, 2.0, 3.0), (3e38, 3e38, 0.0), (3e38, 2.0, -3e38),
                     (0.0, 5.0, 0.0), (1e-30, 1e-30, 0.0), (1e-30, 1e-10, 1e-45), (2.0 ** -75, 2.0 ** -75, 0.0), (2.0 ** -75, 2.0 ** -75, 2.0 ** -149),
                     (1.0, 1.0, 2.0 ** -149), (2.0 ** -100, 2.0 ** -26, 2.0 ** -126)], dtype=np.float32)
    a, b, c = rows.T.copy()
    assert same_bits(fma32(a, b, c), fmaf(a, b, c)).all()


ROWS = [   # B, C1, C2, H, W, Cout, KH, KW, stride, pad
    (2, 16, 0, 6, 7, 5, 3, 3, 1, (1, 1)),
    (1, 3, 2, 9, 8, 4, 2, 5, 2, (0, 2)),
    (1, 2, 0, 9, 9, 3, 7, 7, 1, (3, 3)),
]


def operands(B, C1, C2, H, W, Cout, KH, KW, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(B, C1, H, W, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, KH, KW, generator=g) / math.sqrt((C1 + C2) * KH * KW)
    return x1, x2, w


@pytest.mark.parametrize("B,C1,C2,H,W,Cout,KH,KW,stride,pad", ROWS)
def test_conv_chain_meets_its_deterministic_bound(B, C1, C2, H, W, Cout, KH, KW, stride, pad):
    """y64 and A are the fp64 convolution and its magnitude sum; |y32 - y64| <= (K + 1) u A: K roundings of relative size u on partial sums
    bounded by A (the standard bound gamma_K A, with (K + 1) u >= gamma_K = K u / (1 - K u) for K u < 1 / (K + 1))"""
    x1, x2, w = operands(B, C1, C2, H, W, Cout, KH, KW, 77)
    y32, y64, A = conv_chain_reference(x1, x2, w, stride, pad)
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    true = F.conv2d(xin.double(), w.double(), stride=stride, padding=pad)
    assert y32.dtype == torch.float32 and y32.shape == true.shape
    assert float((y64 - true).abs().max()) <= 1e-13 * float(A.max())
    assert float((A - F.conv2d(xin.double().abs(), w.double().abs(), stride=stride, padding=pad)).abs().max()) <= 1e-13 * float(A.max())
    K = (C1 + C2) * KH * KW
    ratio = float(((y32.double() - y64).abs() / ((K + 1) * U * A)).max())
    print("\nK = %d: worst |y32 - y64| / ((K + 1) u A) = %.4f" % (K, ratio))
    assert 0.0 < ratio <= 1.0
    assert float((y32.double() - y64).abs().max()) > 0.0


def test_convT_chain_meets_its_deterministic_bound():
    g = torch.Generator().manual_seed(78)
    x, w = torch.randn(2, 20, 5, 7, generator=g), torch.randn(20, 9, 2, 2, generator=g) / math.sqrt(20)
    y32, y64, A = convT_chain_reference(x, w)
    true = F.conv_transpose2d(x.double(), w.double(), stride=2)
    assert y32.shape == true.shape == (2, 9, 10, 14)
    assert float((y64 - true).abs().max()) <= 1e-13 * float(A.max())
    ratio = float(((y32.double() - y64).abs() / (21 * U * A)).max())
    assert 0.0 < ratio <= 1.0


def test_chain_depends_on_its_k_order():
    """a 3x3, 16-channel row: the chain walked from k = K - 1 down to 0 differs from the kernel's order in at least one element (in most)
    while both stay inside the bound: the bit-for-bit comparison of the GPU module can fail where every tolerance passes"""
    B, C1, C2, H, W, Cout, KH, KW, stride, pad = ROWS[0]
    x1, x2, w = operands(B, C1, C2, H, W, Cout, KH, KW, 77)
    y32, y64, A = conv_chain_reference(x1, x2, w, stride, pad)
    K = C1 * KH * KW
    back = conv_chain_reference(x1, x2, w, stride, pad, order=range(K - 1, -1, -1))[0]
    differ = int((back != y32).sum())
    print("\nreversed k order: %d of %d elements differ" % (differ, y32.numel()))
    assert differ >= 1
    assert float(((back.double() - y64).abs() / ((K + 1) * U * A)).max()) <= 1.0
    # the two k of one MFMA swapped (lanes 0-31 and 32-63 exchanged): the subtle kind
    swapped = [k ^ 1 for k in range(K)]
    assert K % 2 == 0 and sorted(swapped) == list(range(K))
    sw = conv_chain_reference(x1, x2, w, stride, pad, order=swapped)[0]
    print("half-waves swapped: %d of %d elements differ" % (int((sw != y32).sum()), y32.numel()))
    assert int((sw != y32).sum()) >= 1


# ---- the bias-initialised chain of the direct small-channel kernels (csrc/conv_direct.hip, csrc/conv_stem.hip)
DIRECT_ROWS = [   # B, Cin, H, W, Cout, K, residual
    (2, 1, 3, 4, 3, 3, False),
    (1, 2, 4, 3, 2, 3, True),
    (1, 6, 2, 5, 2, 1, False),
    (1, 3, 1, 1, 2, 3, True),                          # one pixel: eight of nine taps are padding
]


def direct_operands(B, Cin, H, W, Cout, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    return x, w, torch.randn(Cout, generator=g), torch.randn(B, Cout, H, W, generator=g)


@pytest.mark.parametrize("B,Cin,H,W,Cout,K,residual", DIRECT_ROWS)
def test_direct_reference_is_a_scalar_fmaf_loop_from_the_bias(fmaf, B, Cin, H, W, Cout, K, residual):
    """acc = bias[co]; for ci, ky, kx: acc = fmaf(w, x or the padding's 0, acc); then one fp32 addition of the residual -- libm's fmaf, one
    output at a time, against direct_conv_reference, bit for bit"""
    x, w, bias, res = direct_operands(B, Cin, H, W, Cout, K, 91)
    y32, y64, A = direct_conv_reference(x, w, bias, res if residual else None)
    xn, wn, bn, rn = x.numpy(), w.numpy(), bias.numpy(), res.numpy()
    want = np.zeros((B, Cout, H, W), dtype=np.float32)
    R = K // 2
    for b in range(B):
        for co in range(Cout):
            for y in range(H):
                for xx in range(W):
                    acc = np.array([bn[co]], dtype=np.float32)
                    for ci in range(Cin):
                        for ky in range(K):
                            for kx in range(K):
                                yy, xc = y + ky - R, xx + kx - R
                                v = xn[b, ci, yy, xc] if 0 <= yy < H and 0 <= xc < W else np.float32(0)
                                acc = fmaf([wn[co, ci, ky, kx]], [v], acc)
                    want[b, co, y, xx] = acc[0] + rn[b, co, y, xx] if residual else acc[0]
    assert want.dtype == np.float32
    assert same_bits(y32.numpy(), want).all()
    true = F.conv2d(x.double(), w.double(), bias.double(), padding=R) + (res.double() if residual else 0.0)
    assert float((y64 - true).abs().max()) <= 1e-13 * float(A.max())
    assert bool((A >= bias.double().abs().view(1, -1, 1, 1)).all()), "|bias| is part of A"
    # no bias is a chain from +0, the existing form
    assert torch.equal(direct_conv_reference(x, w, None)[0], conv_chain_reference(x, None, w, 1, (R, R))[0])


def test_chain_from_the_bias_is_not_the_chain_plus_the_bias():
    """2 x 2 x 9 x 11 -> 6, 3x3: starting the accumulator at the bias and adding the bias to the finished sum differ (the first rounds
    bias + w0 x0 once, the other w0 x0 and every later partial sum without the bias in it), so a kernel that does the other cannot
    equal the reference by accident; both stay inside the deterministic bound"""
    x, w, bias, _ = direct_operands(2, 2, 9, 11, 6, 3, 92)
    y32, y64, A = direct_conv_reference(x, w, bias)
    after = conv_chain_reference(x, None, w, 1, (1, 1))[0] + bias.view(1, -1, 1, 1)
    assert after.dtype == torch.float32
    differ = int((after != y32).sum())
    print("\nbias first against bias last: %d of %d elements differ" % (differ, y32.numel()))
    assert differ >= 1
    assert float(((y32.double() - y64).abs() / (20 * U * A)).max()) <= 1.0 and float(((after.double() - y64).abs() / (20 * U * A)).max()) <= 1.0
