"""The shared fp32 -> f16 hi/lo split of csrc/common.h (split2_f16: one v_cvt_pk_f16_f32 and two v_fma_mix*_f16 per pair) is the plain form
`hi = (f16)x; lo = (f16)(x - (float)hi)` bit for bit, and the convolution kernels staged with it give the bits they gave before it.

* test_split_bitwise: cf_debug_split_f16 runs both forms in one launch on ~1 M fp32 patterns (every exponent with random mantissas, +-0, the
  fp32 and f16 subnormal ranges, the neighbourhood of 65504, +-inf, NaN).  hi and lo must be bitwise equal wherever the plain result is not
  NaN, and NaN wherever it is.  No pattern is left out.
* test_conv_bits_match_recorded: one small shape per kernel family, without the fp64 statistics atomics (stats_groups=None: those launches
  are run-to-run deterministic), against tests/golden/split_conv_bits.npz, recorded from the commit before the shared split
  (`python tests/test_gpu_split.py --record` on an MI355X with that commit's library).  An output is held as the SHA-256 of its bytes plus
  every STRIDE-th value (the outputs are up to 84 MB; the values say how far off a mismatch is).

Inputs come from seeded CPU generators and, for the deferred normalisation, a coefficient table built on the CPU: nothing but weight packing
and the kernel under test runs on the device."""
import ctypes
import hashlib
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_conv_bits.npz")
STRIDE = 4099        # prime: walks every channel / row / column phase


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def split_patterns():
    """fp32 bit patterns, 2^20 of them (even count: the kernel works on pairs)"""
    g = torch.Generator().manual_seed(7)
    parts = []
    # every exponent (0 = zero / fp32 subnormals ... 255 = inf / NaN) x both signs x 1536 random mantissas
    expo = torch.arange(256, dtype=torch.int64).repeat_interleave(2 * 1536)
    sign = torch.arange(2, dtype=torch.int64).repeat_interleave(1536).repeat(256)
    mant = torch.randint(0, 1 << 23, (expo.numel(),), generator=g, dtype=torch.int64)
    parts.append((sign << 31) | (expo << 23) | mant)
    # specials: +-0, +-inf, quiet / signalling-pattern NaNs, the largest / smallest of each class
    parts.append(torch.tensor([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                               0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000], dtype=torch.int64))
    # f16 subnormal range and the flush boundary below it: exponents 2^-27 .. 2^-13, dense mantissas
    for e in range(127 - 27, 127 - 12):
        m = torch.randint(0, 1 << 23, (8192,), generator=g, dtype=torch.int64)
        s = torch.randint(0, 2, (8192,), generator=g, dtype=torch.int64)
        parts.append((s << 31) | (e << 23) | m)
    # around 65504 (largest f16) and 65520 (where the conversion rounds to inf): every fp32 in [65472, 65552), both signs
    lo_b = int(np.float32(65472.0).view(np.uint32))
    hi_b = int(np.float32(65552.0).view(np.uint32))
    around = torch.arange(lo_b, hi_b, dtype=torch.int64)
    parts += [around, around | (1 << 31)]
    # ties of the hi rounding: values exactly half-way between two f16 numbers (mantissa bits 12..0 = 0x1000), and their fp32 neighbours
    e = torch.randint(127 - 14, 127 + 16, (20000,), generator=g, dtype=torch.int64)
    m10 = torch.randint(0, 1 << 10, (20000,), generator=g, dtype=torch.int64)
    tie = (e << 23) | (m10 << 13) | 0x1000
    parts += [tie, tie - 1, tie + 1, tie | (1 << 31)]
    bits = torch.cat(parts)
    n = 1 << 20
    assert bits.numel() <= n, bits.numel()
    # fill up with uniformly random bit patterns
    fill = torch.randint(0, 1 << 32, (n - bits.numel(),), generator=g, dtype=torch.int64)
    bits = torch.cat([bits, fill])
    return bits.numpy().astype(np.uint32)


def test_split_bitwise(dev):
    from cineflow._lib import lib, check, P, L
    fn = lib().cf_debug_split_f16
    fn.argtypes = [P, P, P, P, P, L, P]
    fn.restype = ctypes.c_int
    bits = split_patterns()
    n = bits.size
    x = torch.from_numpy(bits.view(np.float32).copy()).to(dev)
    outs = [torch.full((n,), 0x5555, dtype=torch.int16, device=dev) for _ in range(4)]
    check(fn(x.data_ptr(), *[o.data_ptr() for o in outs], n, None), "cf_debug_split_f16")
    torch.cuda.synchronize()
    hi_old, lo_old, hi_new, lo_new = [o.cpu().numpy().view(np.uint16) for o in outs]

    def is_nan(h):
        return ((h & 0x7C00) == 0x7C00) & ((h & 0x03FF) != 0)

    # the plain form on the device is the plain form: hi is numpy's round-to-nearest-even conversion (no flushed subnormals)
    with np.errstate(over="ignore", invalid="ignore"):
        want_hi = bits.view(np.float32).astype(np.float16).view(np.uint16)
    ok = ~is_nan(want_hi)
    assert np.array_equal(hi_old[ok], want_hi[ok]) and is_nan(hi_old[~ok]).all()
    for name, old, new in (("hi", hi_old, hi_new), ("lo", lo_old, lo_new)):
        nan = is_nan(old)
        bad = np.flatnonzero((~nan) & (old != new))
        assert bad.size == 0, "%s differs at %d patterns, first x = 0x%08x: plain 0x%04x, shared 0x%04x" % (
            name, bad.size, bits[bad[0]], old[bad[0]], new[bad[0]])
        bad = np.flatnonzero(nan & ~is_nan(new))
        assert bad.size == 0, "%s is NaN in the plain form only at %d patterns, first x = 0x%08x -> 0x%04x" % (name, bad.size, bits[bad[0]], new[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------------------
def _coef(B, C, seed):
    """{mean, scale, shift} table [B, 3, C] as cf_group_norm_coef lays it out, from the CPU generator"""
    mean = randn(B, 1, C, seed=seed) * 0.3
    scale = randn(B, 1, C, seed=seed + 1).abs() * 0.5 + 0.5
    shift = randn(B, 1, C, seed=seed + 2) * 0.3
    return torch.cat([mean, scale, shift], 1).contiguous()


def _f16s(dev, B, C, H, W, Cout, seed):
    from cineflow import ops
    x = randn(B, C, H, W, seed=seed).to(dev)
    w = (randn(Cout, C, 3, 3, seed=seed + 1) / math.sqrt(C * 9)).to(dev)
    b = randn(Cout, seed=seed + 2).to(dev)
    wpk, ws = ops.pack_conv_weight_f16s(w)
    return ops.conv2d_f16s(x, wpk, ws, b, Cout, 3, 3, 1, (1, 1))


def _stream(dev, B, C1, C2, H, W, Cout):
    """STREAM_CASES shapes of test_gpu_ops.py at route level 2 (conv_stream takes every shape it can run)"""
    from cineflow import ops
    from cineflow._lib import lib
    x1 = randn(B, C1, H, W, seed=80).to(dev)
    x2 = randn(B, C2, H, W, seed=81).to(dev) if C2 else None
    w = (randn(Cout, C1 + C2, 3, 3, seed=82) / math.sqrt((C1 + C2) * 9)).to(dev)
    b = randn(Cout, seed=83).to(dev)
    wpk, ws = ops.pack_conv_weight_f16s(w, c1=C1 if (C2 and C1 % 16) else None)
    prev = lib().cf_conv_stream_enable(2)
    try:
        return ops.conv2d_f16s(x1, wpk, ws, b, Cout, 3, 3, 1, (1, 1), x2=x2)
    finally:
        lib().cf_conv_stream_enable(prev)


def _wino(dev, level, slope):
    """the smallest WINO_CASES / prenorm shape of test_gpu_wino.py (480 -> 480 at 16 x 16) on kernel form `level`; slope None: plain, else the
    deferred normalisation with LeakyReLU(slope) or, slope < 0, GELU"""
    from cineflow import ops
    from cineflow._lib import lib
    B, C, H, W, Cout = 2, 480, 16, 16, 480
    x = (randn(B, C, H, W, seed=30) * 1.7 + 0.4).to(dev)
    w = (randn(Cout, C, 3, 3, seed=32) / math.sqrt(C * 9)).to(dev)
    b = randn(Cout, seed=33).to(dev)
    wpk, ws = ops.pack_conv_weight_wino(w)
    prev = lib().cf_conv_wino_enable(level)
    try:
        assert ops.wino_ok(B, C, 0, H, W, Cout, prenorm=slope is not None)
        if slope is None:
            return ops.conv2d_wino(x, wpk, ws, b, Cout)
        return ops.conv2d_wino_prenorm(x, _coef(B, C, 40).to(dev), slope, wpk, ws, b, Cout)
    finally:
        lib().cf_conv_wino_enable(prev)


CASES = {
    "f16s_16x16": lambda dev: _f16s(dev, 2, 16, 16, 16, 16, 10),            # 16 -> 16 at 16 x 16: vector staging (W % 4 == 0)
    "f16s_15x17": lambda dev: _f16s(dev, 2, 16, 15, 17, 16, 20),            # the same layer on the scalar staging path (eight values per task)
    # the smallest STREAM_CASES shape; its 650 tiles are below the 1024 at which conv_stream engages, so it runs conv_f16s with split-aware packing
    "stream_smallest": lambda dev: _stream(dev, 10, 20, 28, 100, 132, 64),
    # the smallest STREAM_CASES shapes that conv_stream itself runs: 32 channels (one m-tile, 1320 tiles of 16 rows, ragged rows and columns)
    # and 64 channels (two m-tiles, 1280 tiles of 8 rows)
    "stream_32": lambda dev: _stream(dev, 33, 32, 0, 120, 132, 32),
    "stream_64": lambda dev: _stream(dev, 20, 64, 0, 128, 128, 64),
}
for _lv in (2, 4, 8):
    CASES["wino%d_plain" % _lv] = lambda dev, lv=_lv: _wino(dev, lv, None)
    CASES["wino%d_lrelu" % _lv] = lambda dev, lv=_lv: _wino(dev, lv, 0.01)
    CASES["wino%d_gelu" % _lv] = lambda dev, lv=_lv: _wino(dev, lv, -1.0)


def _digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(a.tobytes()).hexdigest(), a.reshape(-1)[::STRIDE].copy()


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(GOLDEN_FILE, allow_pickle=False))


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_bits_match_recorded(dev, recorded, name):
    sha, sample = _digest(CASES[name](dev))
    want = recorded[name + ".sample"]
    d = float(np.abs(sample.astype(np.float64) - want.astype(np.float64)).max())
    nbits = int((sample.view(np.uint32) != want.view(np.uint32)).sum())
    assert sha == str(recorded[name + ".sha256"]), "%s: output bits changed (of %d sampled values %d differ, max |diff| %.3e)" % (name, want.size, nbits, d)


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cardiac-segmentation-optical-flow_amd")]
    assert sys.argv[1:2] == ["--record"], "usage: test_gpu_split.py --record [FILE]"
    device = torch.device("cuda:0")
    rec = {}
    for nm in sorted(CASES):
        sha, sample = _digest(CASES[nm](device))
        sha2, _ = _digest(CASES[nm](device))
        assert sha == sha2, "%s is not run-to-run deterministic" % nm
        rec[nm + ".sha256"] = np.array(sha)
        rec[nm + ".sample"] = sample
        print(nm, sha, sample.size)
    np.savez(sys.argv[2] if len(sys.argv) > 2 else GOLDEN_FILE, **rec)
