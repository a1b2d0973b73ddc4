"""The fp32 fused-multiply-add chain that csrc/conv.hip promises ("bit-equivalent to a k-ordered fmaf chain"), on the CPU in numpy, shared by
test_fma_chain_cpu.py (which holds it to libm's fmaf) and test_gpu_conv_f32_routes.py (which holds the kernel to it, bit for bit).  A plain
helper module: no tests live here.

fma32(a, b, c) = the correctly rounded fp32 value of a * b + c.  The product of two fp32 values has 48 significant bits and an exponent far
inside the fp64 range, so it is exact in fp64.  The sum p + c is then taken with TwoSum (s = fl64(p + c) and the exact error e of that
rounding); where e != 0 and the fp64 significand of s is even, s moves one fp64 step towards e: s is now the sum rounded to odd at 53 bits,
and rounding an odd-rounded value of 24 + 2 or more bits to 24 bits (fewer for an fp32 subnormal) gives the correctly rounded result
(Boldo and Melquiond, "Emulation of FMA and correctly rounded sums: proved algorithms using rounding to odd", 2008).  A plain
fl32(fl64(a * b + c)) rounds twice and is wrong where the first rounding lands on an fp32 midpoint: DOUBLE_ROUNDING_TRIPLES.

conv_chain_reference / convT_chain_reference walk k = ci * KH * KW + kh * KW + kw from 0 upwards, the order of conv_igemm_f32_kernel, from an
accumulator of +0, vectorised over every output element.  A tap that falls into the zero padding contributes fma(w, 0, acc) as in the
kernel (which loads 0 there and multiplies): acc unchanged for finite w.  Subnormal products and sums are kept (gradual underflow): numpy
does not flush, and neither may the kernel.

direct_conv_reference is the same walk for the direct small-channel kernels (csrc/conv_direct.hip, csrc/conv_stem.hip), whose accumulator
starts at the bias (`init`) instead of +0: fma(w, x, b) rounds once where fl32(fl32(w x) + b) rounds twice, and the two differ
(test_fma_chain_cpu.py).  Held to those kernels, bit for bit, in test_gpu_direct_conv_chains.py.
"""
import numpy as np
import torch

F32, F64, U64 = np.float32, np.float64, np.uint64


def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def add_round_odd(p, c):
    """p + c of two float64 arrays (broadcast), rounded to odd at 53 bits; non-finite sums pass through"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                # TwoSum: s + err == p + c exactly
        bits = np.ascontiguousarray(s).view(U64)
        fix = (err != 0) & ((bits & U64(1)) == 0) & np.isfinite(s)
        if not fix.any():
            return s
        away = (err > 0) == (s > 0)                    # the exact sum lies beyond s, seen from zero; s != 0 wherever err != 0
        stepped = np.where(away, bits + U64(1), bits - U64(1))
        return np.where(fix, stepped, bits).view(F64)


def fma32(a, b, c):
    """correctly rounded fp32 a * b + c of float32 arrays (module docstring)"""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return add_round_odd(a.astype(F64) * b.astype(F64), c.astype(F64)).astype(F32)


def fma32_plain(a, b, c):
    """fl32(fl64(a * b + c)): rounds twice.  Here to show that fma32 is needed, not to be used."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _double_rounding_triples():
    """(a, b, c) with a * b an fp32 midpoint and c = +-2^-60 pointing at the ODD neighbour: fl64 drops c, the tie then goes to even, fmaf
    goes to odd.  24929 x 673 = 2^24 + 1 (neighbours 1 even, 1 + 2^-23 odd: c > 0); 5592407 x 3 = 2^24 + 5 (1 + 2^-22 even below,
    1 + 3 x 2^-23 odd above: c > 0); 31 x 1082401 = 2^25 - 1 (2 - 2^-24: 2 - 2^-23 odd below, 2 even above: c < 0).  All times 2^-24,
    each with both signs of the product and both ways of making that sign."""
    rows = []
    for a, b, scale, c in ((24929, 673, 2.0 ** -24, 2.0 ** -60), (5592407, 3, 2.0 ** -24, 2.0 ** -60), (31, 1082401, 2.0 ** -24, -2.0 ** -60)):
        assert a * b in (2 ** 24 + 1, 2 ** 24 + 5, 2 ** 25 - 1)
        for sign in (1.0, -1.0):
            rows.append((float(a), sign * b * scale, sign * c))
            rows.append((-float(a), -sign * b * scale, sign * c))
    return np.array(rows, dtype=F32)


DOUBLE_ROUNDING_TRIPLES = _double_rounding_triples()


def _chain(xp, w64, stride, Ho, Wo, order, init=None):
    """xp float64 [B, Cin, Hp, Wp] (already zero padded), w64 float64 [Cout, Cin, KH, KW] -> (y32, y64, A) float arrays [B, Cout, Ho, Wo];
    init: float32 [Cout], the value the accumulator starts from (None: +0) -- part of y64, its magnitude part of A"""
    B = xp.shape[0]
    Cout, Cin, KH, KW = w64.shape
    acc = np.zeros((B, Cout, Ho, Wo), dtype=F64)       # holds fp32 values
    if init is not None:
        init = np.asarray(init)
        assert init.dtype == F32 and init.shape == (Cout,)
        acc += init.astype(F64)[None, :, None, None]
    y64 = acc.copy()
    A = np.abs(acc)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in (range(Cin * KH * KW) if order is None else order):
            ci, r = divmod(int(k), KH * KW)
            kh, kw = divmod(r, KW)
            xs = xp[:, ci, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride][:, None]
            p = w64[:, ci, kh, kw][None, :, None, None] * xs       # exact
            acc = add_round_odd(p, acc).astype(F32).astype(F64)
            y64 += p
            A += np.abs(p)
    return acc.astype(F32), y64, A


def conv_chain_reference(x1, x2, w, stride, pad, order=None, init=None):
    """conv2d of cat[x1, x2] (x2 may be None) with w [Cout, Cin, KH, KW]: (y32, y64, A) as torch tensors [B, Cout, Ho, Wo] --
    the fp32 fmaf chain in the kernel's k order (or in `order`, a permutation of range(K)), the fp64 sum of the exact products and
    A = sum |w| |x|.  init (float32 [Cout] or None for +0): the accumulator's first value, a bias the chain STARTS from (as the direct
    kernels do) instead of one added to the finished sum; y64 includes it and A its magnitude."""
    x = _np(x1, F64) if x2 is None else np.concatenate([_np(x1, F64), _np(x2, F64)], 1)
    w64 = _np(w, F64)
    B, Cin, H, W = x.shape
    Cout, Cw, KH, KW = w64.shape
    assert Cw == Cin
    ph, pw = pad
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    assert Ho > 0 and Wo > 0
    xp = np.zeros((B, Cin, H + 2 * ph, W + 2 * pw), dtype=F64)
    xp[:, :, ph:ph + H, pw:pw + W] = x
    init = None if init is None else _np(init)
    return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in _chain(xp, w64, stride, Ho, Wo, order, init))


def direct_conv_reference(x, w, bias, res=None):
    """the direct small-channel kernels (csrc/conv_direct.hip, csrc/conv_stem.hip): 3x3 pad 1 or 1x1 pad 0, stride 1, the chain over
    ci, then ky, then kx from an accumulator that starts at the bias (float32 [Cout] or None); res (same shape as the output) is added
    afterwards as one rounded fp32 addition, fl32(y32 + res), as conv3x3_small_cout_kernel does: (y32, y64, A), res in all three"""
    K = w.shape[-1]
    assert tuple(w.shape[2:]) in ((3, 3), (1, 1))
    y32, y64, A = conv_chain_reference(x, None, w, 1, (K // 2, K // 2), init=bias)
    if res is not None:
        res = torch.from_numpy(_np(res, F32))
        assert res.shape == y32.shape
        with np.errstate(invalid="ignore", over="ignore"):
            y32 = y32 + res                            # one fp32 addition per element
        y64, A = y64 + res.double(), A + res.double().abs()
    assert y32.dtype == torch.float32
    return y32, y64, A


def convT_chain_reference(x, w, order=None):
    """ConvTranspose2d(kernel 2, stride 2) of x [B, Cin, H, W] with w [Cin, Cout, 2, 2], no bias: the chain over k = ci of the GEMM rows
    m = co * 4 + dy * 2 + dx, scattered to [B, Cout, 2 H, 2 W] (out[b, co, 2 y + dy, 2 x + dx]): (y32, y64, A)"""
    x64, w64 = _np(x, F64), _np(w, F64)
    B, Cin, H, W = x64.shape
    Cout = w64.shape[1]
    assert w64.shape == (Cin, Cout, 2, 2)
    rows = w64.reshape(Cin, Cout * 4).T.reshape(Cout * 4, Cin, 1, 1)       # row m = co * 4 + dy * 2 + dx
    out = []
    for t in _chain(x64, rows, 1, H, W, order):
        t = t.reshape(B, Cout, 2, 2, H, W).transpose(0, 1, 4, 2, 5, 3).reshape(B, Cout, 2 * H, 2 * W)
        out.append(torch.from_numpy(np.ascontiguousarray(t)))
    return tuple(out)
