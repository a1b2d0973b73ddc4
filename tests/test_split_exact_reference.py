"""CPU checks of the row-Winograd split-exact reference (tests/_split_exact.py) that the GPU table test_gpu_wino_stream_routes.py holds
conv_wino.hip to: the reference itself against an fp64 convolution, the host packing against the reference's operands, and the proof that
the GPU bar can fail; then the same for the composed Conv3d / ConvTranspose layer references (tests/_conv3d_layer_refs.py) that
test_gpu_conv3d_layer_routes.py holds the layers to.  No GPU and no built library: the host packers run on CPU tensors."""
import math

import pytest
import torch
import torch.nn.functional as F

from _conv3d_layer_refs import (LAYER_ROWS, T_ROWS, composed_reference, host_scales, layer_operands, layer_reference, lrow_id, shifted,
                                t_host_scales, t_operands, t_reference, t_swaps, trow_id)
from _split_exact import SPLIT_BAR, randn, ratio, wino_scale, wino_split_reference, wino_split_u, wino_unpack

# B, C1, C2, H, W, Cout: 16-wide maps, two inputs with a split that is not a chunk multiple, a channel tail, three tile columns, one row
SHAPES = [
    (2, 32, 0, 8, 16, 16),
    (1, 20, 28, 4, 32, 24),
    (2, 81, 0, 8, 32, 8),
    (1, 128, 0, 16, 32, 16),
    (1, 7, 0, 1, 96, 5),
]


def operands(B, C1, C2, H, W, Cout, seed):
    x = randn(B, C1 + C2, H, W, seed=seed) * 1.3 + 0.2
    w = randn(Cout, C1 + C2, 3, 3, seed=seed + 1) / math.sqrt((C1 + C2) * 9)
    b = randn(Cout, seed=seed + 2)
    return x, w, b


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wino_reference_is_the_convolution(shape):
    """Each operand carries <= 2^-22 relative error after the hi/lo split (fp16 hi: 2^-11, fp16 lo of the remainder: 2^-11 of that; the fp32
    rounding of V and of 2^s G w adds 2^-24 each) and A bounds the sum of the products' magnitudes, so to first order
    |y3 - true| <= 2 x 2^-22 A = 2^-21 A; the bar is 2^-20 A.  The Winograd algebra, the zero padding of rows and columns and the 2^-s scale
    are all wrong by far more than that if wrong at all."""
    x, w, b = operands(*shape, seed=sum(shape))
    r = wino_split_reference(x, w, b, wino_scale(w))
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert float((r["true"] - want).abs().max()) <= 1e-12
    assert r["y3"].shape == want.shape and bool((r["A"] > 0).all())
    got = ratio(r["y3"], want, r["A"])
    assert got <= 2.0 ** -20, got
    # hi x hi alone is an fp16 convolution: 2^-11 relative per operand
    assert 2.0 ** -20 < ratio(r["y1"], want, r["A"]) <= 3 * 2.0 ** -11


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wino_bar_can_fail(shape):
    """what the GPU rows assert per launch, on the reference alone: the one-term result and the result without the last input channel both
    miss the 2^-18 A bar against y3"""
    x, w, b = operands(*shape, seed=sum(shape))
    r = wino_split_reference(x, w, b, wino_scale(w))
    bar = SPLIT_BAR * r["A"]
    assert ratio(r["y1"], r["y3"], bar) > 1.0
    assert ratio(r["y3"] - r["d3"], r["y3"], bar) > 1.0
    assert ratio(r["y1"] - r["d1"], r["y1"], bar) > 1.0
    # the last channel's contribution is exactly what zeroing that channel removes
    x0 = x.clone()
    x0[:, -1] = 0
    r0 = wino_split_reference(x0, w, b, wino_scale(w))
    assert float((r["y3"] - r["d3"] - r0["y3"]).abs().max()) <= 1e-12 * float(r["A"].max())


@pytest.mark.parametrize("Cout,C1,C2", [(128, 32, 0), (224, 81, 0), (480, 48, 0), (128, 20, 28), (224, 100, 60)])
def test_pack_conv_weight_wino_holds_the_reference_operands(Cout, C1, C2):
    """un-permuting the packed tensor gives exactly the Uh, Ul of the reference (so the kernel multiplies what the reference multiplies),
    with zeros in every padded m-tile row and every padded channel, x1's channels padded to whole chunks when the split is not one"""
    from cineflow import ops
    w = randn(Cout, C1 + C2, 3, 3, seed=Cout + C1) / math.sqrt((C1 + C2) * 9)
    wpk, s = ops.pack_conv_weight_wino(w, c1=C1 if C2 else None)
    assert s == wino_scale(w) and wpk.dtype == torch.float16
    uh, ul = wino_split_u(w, s)
    split = C2 > 0 and C1 % 16 != 0
    c1p = (C1 + 15) // 16 * 16 if split else C1
    nchunk = (c1p + C2 + 15) // 16 if split else (C1 + C2 + 15) // 16
    rows = 128 * ((Cout + 127) // 128)
    assert wpk.numel() == 2 * rows * nchunk * 16 * 12
    hi, lo = wino_unpack(wpk, Cout, nchunk)
    for got, want in ((hi, uh), (lo, ul)):
        full = torch.zeros(rows, nchunk * 16, 3, 4, dtype=torch.float64)
        full[:Cout, :C1] = want[:, :C1]
        full[:Cout, c1p:c1p + C2] = want[:, C1:]
        assert torch.equal(got, full)
    assert bool((hi[Cout:] == 0).all()) and bool((lo[Cout:] == 0).all())
    assert bool((hi[:, c1p + C2:] == 0).all()) and bool((hi[:, C1:c1p] == 0).all())
    # the split loses nothing an fp32 accumulator could hold: hi + lo is 2^s G w to 2^-22 relative (2^-21 asserted), or to half the spacing
    # of fp16 subnormals (2^-25) where lo falls among them -- 2^-34 of the largest operand
    G = torch.tensor(ops._WINO_G, dtype=torch.float64)
    U = torch.einsum("pk,ocyk->ocyp", G, w.double()) * 2.0 ** s
    assert bool(((uh + ul - U).abs() <= 2.0 ** -21 * U.abs() + 2.0 ** -25).all())
    assert 512.0 <= float(U.abs().max()) < 1024.0


# ---- the composed Conv3d layer reference ------------------------------------------------------------------------------------------------------
# C, Cout, D, H, W, kernel, stride: every stride pair of the layer table, odd and even depth, no depth taps, one plane
COMPOSED_SHAPES = [
    (40, 48, 5, 12, 20, (3, 3, 3), (1, 1, 1)),
    (40, 48, 5, 13, 11, (3, 3, 3), (2, 2, 2)),
    (40, 48, 4, 12, 20, (3, 3, 3), (2, 2, 2)),
    (24, 40, 4, 12, 20, (3, 3, 3), (1, 2, 2)),
    (24, 40, 5, 12, 20, (3, 3, 3), (2, 1, 1)),
    (24, 40, 3, 12, 20, (1, 3, 3), (1, 2, 2)),
    (24, 40, 1, 6, 12, (3, 3, 3), (1, 1, 1)),
    (24, 40, 5, 9, 7, (3, 1, 1), (1, 1, 1)),
]


def _grid(t, bits):
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]) + "_k%d%d_s%d%d" % (s[5][0], s[5][1], s[6][0], s[6][1]))
def test_composed_reference_is_the_3d_reference_when_the_scales_agree(shape):
    """With one scale exponent for every tap the per-tap sum is the 3-D split_reference of test_gpu_conv3d_routes.py term for term, summed
    in another order.  On operands from a coarse grid (x in multiples of 2^-10 below 8, w in multiples of 2^-12: every product a multiple
    of 2^-11 after the 2^s scaling, every partial sum below 2^25, 36 bits) float64 holds every partial sum exactly, so the order cannot
    matter and the two must agree to the last bit -- y3, y1, A, d3 and z3; the grid still leaves both lo halves non-zero.  On randn
    operands the orders differ by fp64 rounding alone: 2^-40 A, where the GPU bar is 2^-18 A."""
    from cineflow import ops
    from test_gpu_conv3d_routes import split_reference as reference_3d
    C, Cout, D, H, W, k, st = shape
    pad = tuple(v // 2 for v in k)
    conv = lambda a, m: F.conv3d(a, m, stride=st, padding=pad)
    seed = 31 * sum(shape[:5]) + k[0] + st[0]
    x = randn(2, C, D, H, W, seed=seed)
    w = randn(Cout, C, *k, seed=seed + 1) / math.sqrt(C * k[0] * k[1] * k[2])
    b = randn(Cout, seed=seed + 2)
    for exact in (True, False):
        if exact:
            x, w, b = _grid(x.clamp(-7.5, 7.5), 10), _grid(w, 12), _grid(b, 10)
        s = ops._scaled_split(w.reshape(Cout, C, -1), 16, 2)[2]
        want = reference_3d(x, w, b, s, conv)
        got = composed_reference(x, w, b, (s,) * k[0], st)
        assert set(got) == set(want)
        if exact:
            xh = x.half().float()
            assert bool(((x - xh) != 0).any()) and bool(((x - xh).half().float() == x - xh).all())
        for key in want:
            assert got[key].shape == want[key].shape
            if exact:
                assert torch.equal(got[key], want[key]), key
            else:
                assert ratio(got[key], want[key], want["A"]) <= 2.0 ** -40, key
    # two different exponents: the taps' sums carry their own 2^-s (the scaled operands differ, the values do not, outside fp16's subnormals)
    s2 = (s, s - 2, s)[:k[0]] if k[0] == 3 else (s - 2,)
    other = composed_reference(x, w, b, s2, st)
    assert ratio(other["y3"], want["y3"], want["A"]) <= 2.0 ** -20 and ratio(other["true"], want["true"], want["A"]) == 0.0


@pytest.mark.parametrize("row", LAYER_ROWS, ids=lrow_id)
def test_layer_bar_can_fail(row):
    """what the GPU rows assert of the device output, on the reference alone and on the very inputs of each row: the one-term result, the
    result without the last input channel, without depth tap 0 (kd = 3 and D > 1) and the result one plane off along depth each miss the
    2^-18 A bar against y3 somewhere.  A condition on the inputs: a row that does not meet it gets another seed or weight scale."""
    x, w, b = layer_operands(row)
    r = layer_reference(row, host_scales(row, w))
    bar = SPLIT_BAR * r["A"]
    assert bool((r["A"] > 0).all()) and ratio(r["y3"], r["true"], r["A"]) <= 2.0 ** -20
    assert ratio(r["y1"], r["y3"], bar) > 1.0
    assert ratio(r["y3"] - r["d3"], r["y3"], bar) > 1.0
    if row.k[0] == 3:
        if row.D > 1:
            assert ratio(r["y3"] - r["z3"], r["y3"], bar) > 1.0
        else:
            assert float(r["z3"].abs().max()) == 0.0
    if r["y3"].shape[2] > 1:
        assert ratio(shifted(r["y3"]), r["y3"], bar) > 1.0
    # the last channel's contribution is exactly what zeroing that channel removes
    if row.n in (4, 6, 10):
        x0 = x.clone()
        x0[:, -1] = 0
        r0 = composed_reference(x0, w, b, host_scales(row, w), row.stride)
        assert ratio(r["y3"] - r["d3"], r0["y3"], r["A"]) <= 2.0 ** -40


@pytest.mark.parametrize("row", T_ROWS, ids=trow_id)
def test_transposed_layer_bar_can_fail(row):
    """the same for the transposed rows: one term, a dropped last input channel, and the two interleaved positions (depth taps of a
    (2,2,2) kernel, sub-rows / sub-columns of an anisotropic 2-D one) exchanged"""
    x, w, b = t_operands(row)
    r = t_reference(row, t_host_scales(row, w))
    want = (F.conv_transpose3d if row.dims == 3 else F.conv_transpose2d)(x.double(), w.double(), None if b is None else b.double(), stride=row.k)
    assert float((r["true"] - want).abs().max()) <= 1e-12
    bar = SPLIT_BAR * r["A"]
    assert bool((r["A"] > 0).all()) and ratio(r["y3"], r["true"], r["A"]) <= 2.0 ** -20
    assert ratio(r["y1"], r["y3"], bar) > 1.0
    assert ratio(r["y3"] - r["d3"], r["y3"], bar) > 1.0
    if row.dims == 3:
        assert ratio(shifted(r["y3"]), r["y3"], bar) > 1.0
    swaps = t_swaps(row, r["y3"])
    assert bool(swaps) == (row.k[0] == 2 or row.dims == 2)
    for name, y in swaps.items():
        assert ratio(y, r["y3"], bar) > 1.0, name
