"""CPU checks of the row-Winograd split-exact reference (tests/_split_exact.py) that the GPU table test_gpu_wino_stream_routes.py holds
conv_wino.hip to: the reference itself against an fp64 convolution, the host packing against the reference's operands, and the proof that
the GPU bar can fail.  No GPU and no built library: pack_conv_weight_wino runs on CPU tensors."""
import math

import pytest
import torch
import torch.nn.functional as F

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
