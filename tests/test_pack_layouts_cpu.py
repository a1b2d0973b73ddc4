"""The three weight packers of cineflow.ops against naive loop references written straight from their docstrings, as bytes, on CPU tensors.

f16 packers (pack_conv_weight_f16s, pack_conv3d_weight_f16s): element [m-tile][chunk][tap][kstep][part][lane = h*32 + r][j] holds
2^s * W[mt*32 + r][c][tap] for the padded channel c = chunk*CK + kstep*16 + 8h + j (the 3-D packer: CK = 16, one kstep), part 0 = fp16(v),
part 1 = fp16(v - fp16(v)).  Winograd packer: [m-tile][chunk][step = ky*4 + pos][part][lane][j] of U = G w along kx, computed in fp64.
Rows past Cout and padded channels are zero; with a split c1 (0 < c1 < Cin, c1 % CK != 0) the first c1 channels are padded to whole
chunks on their own and the others follow.  s = clamp(floor(log2(1024 / max|.|)), -24, 24), 0 for an all-zero weight.
The shapes are the smallest that reach every branch: Cout <= 32 (one m-tile) and > 32 (an even count), CK 16 and 32, no split, a split
at a chunk-interior channel, taps 1 / 5 / 9 / 27, the Winograd packer's 128-channel blocks (Cout = 130: two blocks, 126 rows padded)."""
import math

import numpy as np
import pytest
import torch

from cineflow import ops

G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def randw(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.1


def exponent(m):
    return max(-24, min(24, int(math.floor(math.log2(1024.0 / m))))) if m > 0 else 0


def source_channel(c, cin, ck, c1):
    """padded channel -> channel of the weight, or None for padding"""
    if c1 is not None and 0 < c1 < cin and c1 % ck:
        c1p = (c1 + ck - 1) // ck * ck
        if c < c1p:
            return c if c < c1 else None
        c = c1 + (c - c1p)
    return c if c < cin else None


def nchunks(cin, ck, c1):
    if c1 is not None and 0 < c1 < cin and c1 % ck:
        return (c1 + ck - 1) // ck + (cin - c1 + ck - 1) // ck
    return (cin + ck - 1) // ck


def loop_pack(wmat, s, ck, nmt, c1, kstep_inside_tap):
    """wmat [Cout, Cin, nstep] float64 numpy (exact values) -> the packed fp16 vector.  kstep_inside_tap: the 2-D f16 packer's order
    [mt][chunk][tap][kstep][part][h][r][j]; else [mt][chunk][step][part][h][r][j] with CK = 16"""
    cout, cin, nstep = wmat.shape
    nks = ck // 16 if kstep_inside_tap else 1
    nchunk = nchunks(cin, ck, c1)
    out = np.zeros((nmt, nchunk, nstep, nks, 2, 2, 32, 8), dtype=np.float16)
    scale = np.float64(2.0) ** s
    for mt in range(nmt):
        for r in range(32):
            co = mt * 32 + r
            if co >= cout:
                continue
            for chunk in range(nchunk):
                for ks in range(nks):
                    for h in range(2):
                        for j in range(8):
                            ci = source_channel(chunk * ck + ks * 16 + 8 * h + j, cin, ck, c1)
                            if ci is None:
                                continue
                            for t in range(nstep):
                                v = np.float32(wmat[co, ci, t] * scale)
                                hi = np.float16(v)
                                out[mt, chunk, t, ks, 0, h, r, j] = hi
                                out[mt, chunk, t, ks, 1, h, r, j] = np.float16(v - np.float32(hi))
    return out.reshape(-1)


def same_bytes(packed, want):
    assert packed.dtype == torch.float16 and packed.numel() == want.size
    assert packed.numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("shape,c1,zero", [((40, 20, 3, 3), None, False), ((40, 20, 3, 3), 12, False), ((8, 40, 1, 1), None, False),
                                           ((8, 40, 1, 5), 24, False), ((40, 20, 3, 3), None, True)])
def test_pack_conv_weight_f16s_matches_its_docstring(shape, c1, zero):
    w = torch.zeros(shape) if zero else randw(*shape, seed=3)
    cout, cin, kh, kw = shape
    ck = 16 if (kh, kw) == (3, 3) else 32
    nmt = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    s = exponent(float(w.abs().max()))
    packed, got_s = ops.pack_conv_weight_f16s(w, c1=c1)
    assert got_s == s and (s == 0) == zero
    same_bytes(packed, loop_pack(w.reshape(cout, cin, kh * kw).double().numpy(), s, ck, nmt, c1, True))


@pytest.mark.parametrize("c1", [None, 12])
def test_pack_conv_weight_wino_matches_its_docstring(c1):
    cout, cin = 130, 20
    w = randw(cout, cin, 3, 3, seed=4)
    wn = w.double().numpy()
    U = np.zeros((cout, cin, 3, 4))
    for pos in range(4):
        for kx in range(3):
            U[..., pos] += G[pos][kx] * wn[..., kx]
    s = exponent(float(np.abs(U).max()))
    packed, got_s = ops.pack_conv_weight_wino(w, c1=c1)
    assert got_s == s
    same_bytes(packed, loop_pack(U.reshape(cout, cin, 12), s, 16, 4 * ((cout + 127) // 128), c1, False))


@pytest.mark.parametrize("shape,c1", [((40, 20, 3, 3, 3), 12), ((8, 20, 1, 3, 3), None)])
def test_pack_conv3d_weight_f16s_matches_its_docstring(shape, c1):
    w = randw(*shape, seed=5)
    cout, cin, kd = shape[:3]
    nmt = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    s = exponent(float(w.abs().max()))
    packed, got_s = ops.pack_conv3d_weight_f16s(w, c1=c1)
    assert got_s == s
    same_bytes(packed, loop_pack(w.reshape(cout, cin, kd * 9).double().numpy(), s, 16, nmt, c1, False))
