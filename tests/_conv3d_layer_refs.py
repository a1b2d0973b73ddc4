"""Shapes and fp64 references of the Conv3d / ConvTranspose layer tables (test_gpu_conv3d_layer_routes.py), checked on the CPU by
test_split_exact_reference.py; the probe pairs are also what test_reference_import_3d.py asks cf_conv3d_f16s_ok.  A plain helper module:
no tests live here.

Composed reference.  nn.Conv3d's composition runs one 2-D convolution per depth tap dz, each on its own packing with its own scale
exponent s_dz, and accumulates the taps through the 2-D kernel's residual input.  The exact operands of tap dz are
    wh_dz, wl_dz = split_w(w[:, :, dz], s_dz)        xh, xl = split_x(x)
    y3_dz = 2^-s_dz (conv(xh, wl_dz) + conv(xl, wh_dz) + conv(xh, wh_dz))
    y3 = b + sum_dz y3_dz         A = |b| + sum_dz 2^-s_dz conv(|xh| + |xl|, |wh_dz| + |wl_dz|)
evaluated in float64.  Which output planes a tap reaches is never written down here: conv is F.conv3d with the layer's stride and padding
on a 5-D weight that is zero outside tap dz, so the placement is PyTorch's, not a restatement of nn.py's slices.  A native row is the same
formula with one scale for every tap (the 3-D packing has one).  Scaling by 2^s commutes with the fp16 rounding only outside the
subnormal range, so the scales are an argument: the GPU tests read them from the layer, the CPU tests from the host packers.

Bar.  The 2-D kernel's accumulator holds one tap's sum (n MFMAs per term, three terms); the composition adds the stored sum of the taps
before it in the epilogue, one more fp32 rounding per tap after the first, each bounded by u A with u = 2^-24: (3 n + 1) kd u A with
certainty, sqrt of that count as a random walk.  The widest rows here have 9 chunks x 9 in-plane taps = 81 MFMAs per term and tap, the
same count per output as the native kernel's table (test_gpu_conv3d_routes.py), whose reasoning carries over: past the 63 steps for
which 2^-18 A = 64 u A (SPLIT_BAR) is certain, far inside the random-walk range.  The layers are held to SPLIT_BAR unchanged; the
worst ratio measured on any row is 0.05 (profiles/conv3d_layer_table.md)."""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from _split_exact import randn, split_w, split_x

# ---- the probe's declines, both sides -------------------------------------------------------------------------------------------------------
# B, C1, C2, D, H, W, Cout, KD, KH, stride_d, stride_hw: (what, declined shape, the nearest taken shape)
PROBE_PAIRS = [
    ("a", (1, 24, 0, 4, 128, 128, 40, 1, 3, 1, 1), (1, 24, 0, 4, 128, 127, 40, 1, 3, 1, 1)),          # no depth taps, 65536 output voxels
    ("a_s2", (1, 24, 0, 4, 256, 256, 40, 1, 3, 1, 2), (1, 24, 0, 4, 256, 254, 40, 1, 3, 1, 2)),
    ("b", (1, 20, 0, 4, 256, 256, 24, 3, 3, 1, 2), (1, 20, 0, 4, 256, 254, 24, 3, 3, 1, 2)),          # in-plane stride 2 at depth stride 1
    ("c", (2, 136, 0, 3, 8, 10, 40, 3, 3, 1, 1), (2, 128, 0, 3, 8, 10, 40, 3, 3, 1, 1)),              # < 512 workgroups, nchunk * KD = 27 > 24
    ("c_sd2", (2, 136, 0, 4, 8, 10, 40, 3, 3, 2, 2), (2, 128, 0, 4, 8, 10, 40, 3, 3, 2, 2)),
    ("c_x2", (2, 72, 64, 3, 8, 10, 40, 3, 3, 1, 1), (2, 64, 64, 3, 8, 10, 40, 3, 3, 1, 1)),           # x1 padded to 5 chunks: 9 * 3 = 27
    ("c_kd1", (2, 400, 0, 3, 8, 10, 40, 1, 3, 1, 1), (2, 384, 0, 3, 8, 10, 40, 1, 3, 1, 1)),          # 25 chunks without depth taps
    ("geometry", (1, 16, 0, 3, 130, 1, 24, 3, 3, 1, 1), (1, 16, 0, 3, 40, 1, 24, 3, 3, 1, 1)),        # a tall one-column tile
    # class (c) again, for the layer rows below whose shape is none of the above
    ("c_odd", (2, 136, 0, 5, 9, 7, 40, 3, 3, 2, 2), (2, 128, 0, 5, 9, 7, 40, 3, 3, 2, 2)),
    ("c_d1", (2, 136, 0, 1, 8, 10, 40, 3, 3, 1, 1), (2, 128, 0, 1, 8, 10, 40, 3, 3, 1, 1)),
    ("c_6x8", (2, 136, 0, 3, 6, 8, 40, 3, 3, 1, 1), (2, 128, 0, 3, 6, 8, 40, 3, 3, 1, 1)),
]
PAIR = {name: (declined, taken) for name, declined, taken in PROBE_PAIRS}

# ---- Conv3d layer rows ---------------------------------------------------------------------------------------------------------------------
# pair: the PROBE_PAIRS entry whose declined shape the row is; None: no native kernel has the row's kernel size; "native": the row runs native
LRow = namedtuple("LRow", "n B C1 C2 D H W Cout k stride pair")
LAYER_ROWS = [
    LRow(1, 1, 24, 0, 4, 128, 128, 40, (1, 3, 3), (1, 1, 1), "a"),           # one tap, no accumulate; all planes are one 2-D batch
    LRow(2, 1, 24, 0, 4, 256, 256, 40, (1, 3, 3), (1, 2, 2), "a_s2"),
    LRow(3, 1, 20, 0, 4, 256, 256, 24, (3, 3, 3), (1, 2, 2), "b"),           # the stride-2 2-D kernel with res aliasing out; both depth borders
    LRow(4, 2, 136, 0, 3, 8, 10, 40, (3, 3, 3), (1, 1, 1), "c"),             # several planes per workgroup with res aliasing out; 136 = 8 * 16 + 8
    LRow(5, 2, 136, 0, 4, 8, 10, 40, (3, 3, 3), (2, 2, 2), "c_sd2"),         # even D: the last output plane loses its far tap; strided slices
    LRow(6, 2, 136, 0, 5, 9, 7, 40, (3, 3, 3), (2, 2, 2), "c_odd"),          # odd sizes, Do = 3
    LRow(7, 2, 72, 64, 3, 8, 10, 40, (3, 3, 3), (1, 1, 1), "c_x2"),          # x2 and a split-aware packing per tap
    LRow(8, 2, 136, 0, 1, 8, 10, 40, (3, 3, 3), (1, 1, 1), "c_d1"),          # D = 1: only the centre tap runs
    LRow(9, 1, 16, 0, 3, 130, 1, 24, (3, 3, 3), (1, 1, 1), "geometry"),      # a one-column map
    LRow(10, 2, 24, 0, 5, 9, 7, 40, (3, 1, 1), (1, 1, 1), None),             # 1x1 taps: a kernel neither native kernel takes
    LRow(11, 1, 24, 0, 4, 128, 127, 40, (1, 3, 3), (1, 1, 1), "native"),     # row 1's neighbour: a layer that silently stays composed fails here
    LRow(12, 2, 136, 0, 3, 6, 8, 40, (3, 3, 3), (1, 1, 1), "c_6x8"),         # row 4 on 6x8 maps: two planes per workgroup at stride 1 (8x10 has one)
]
# images per workgroup of the rows' 2-D tap calls (cf_conv2d_f16s_route), by planes in the call; rows not named: 1
TAP_NIMG = {5: {2: 2, 1: 1}, 6: {3: 3, 2: 2}, 10: {5: 2, 4: 2}, 12: {3: 2, 2: 2}}


def lrow_id(r):
    return "row%d_k%d%d_s%d%d" % (r.n, r.k[0], r.k[1], r.stride[0], r.stride[1])


def probe_args(r):
    return (r.B, r.C1, r.C2, r.D, r.H, r.W, r.Cout, r.k[0], r.k[1], r.stride[0], r.stride[1])


@functools.lru_cache(maxsize=None)
def layer_operands(r):
    """(x, w, b) of a row; row 11 has row 1's weights and row 1's input without its last column"""
    if r.n == 11:
        x, w, b = layer_operands(LAYER_ROWS[0])
        return x[..., :r.W].contiguous(), w, b
    C = r.C1 + r.C2
    seed = 7000 + 100 * r.n
    x = randn(r.B, C, r.D, r.H, r.W, seed=seed)
    w = randn(r.Cout, C, *r.k, seed=seed + 1) / math.sqrt(C * r.k[0] * r.k[1] * r.k[2])
    if r.n == 6:
        w[:, :, 0] *= 0.25              # one row whose taps are packed with different scale exponents
    return x, w, randn(r.Cout, seed=seed + 2)


def host_scales(r, w):
    """the scale exponents the layer's packings will have, from the host packers the layer itself calls (they run on CPU tensors)"""
    from cineflow import ops
    if r.pair == "native":
        return (ops.pack_conv3d_weight_f16s(w)[1],) * r.k[0]
    return tuple(ops.pack_conv_weight_f16s(w[:, :, dz].contiguous())[1] for dz in range(r.k[0]))


def _three(conv, xh, xl, wh, wl):
    return conv(xh, wl) + conv(xl, wh) + conv(xh, wh)


def composed_reference(x, w, b, scales, stride):
    """fp64 {y3, y1, true, A, d3 = the last input channel's split-exact contribution, z3 = depth tap 0's (kd = 3 only)} of the layer
    Conv3d(kernel w.shape[2:], stride, padding k // 2) whose depth tap dz was packed with the scale exponent scales[dz]"""
    kd = w.shape[2]
    assert len(scales) == kd
    pad = tuple(k // 2 for k in w.shape[2:])
    conv = lambda a, m: F.conv3d(a, m, stride=stride, padding=pad)
    xh, xl = split_x(x)
    xa = xh.abs() + xl.abs()
    c = x.shape[1] - 1
    bb = (b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)).view(1, -1, 1, 1, 1)
    y3 = y1 = A = d3 = z3 = 0.0
    for dz in range(kd):
        th, tl = split_w(w[:, :, dz], scales[dz])
        wh, wl = torch.zeros(w.shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64)
        wh[:, :, dz], wl[:, :, dz] = th, tl                 # zero outside tap dz: F.conv3d places the tap's planes
        sc = 2.0 ** -scales[dz]
        t3 = sc * _three(conv, xh, xl, wh, wl)
        y3 = y3 + t3
        y1 = y1 + sc * conv(xh, wh)
        A = A + sc * conv(xa, wh.abs() + wl.abs())
        d3 = d3 + sc * _three(conv, xh[:, c:], xl[:, c:], wh[:, c:], wl[:, c:])
        if dz == 0:
            z3 = t3
    r = dict(y3=y3 + bb, y1=y1 + bb, true=conv(x.double(), w.double()) + bb, A=A + bb.abs(), d3=d3)
    if kd == 3:
        r["z3"] = z3
    return r


@functools.lru_cache(maxsize=None)
def layer_reference(r, scales):
    """composed_reference of a row's operands, computed once per (row, scales) and shared; callers leave it unchanged"""
    x, w, b = layer_operands(r)
    return composed_reference(x, w, b, scales, r.stride)


def shifted(y):
    """y one plane along depth (cyclic): what a layer that places its planes one off would return; defined for more than one plane"""
    assert y.shape[2] > 1
    return torch.roll(y, 1, dims=2)


def in_range_taps(r):
    """[(sample, dz, first output plane, [input planes])] in the order the composition must issue them: per sample the centre tap, then
    the others ascending; a tap with no output plane in range is absent.  Enumerated plane by plane, no closed form."""
    kd, sd = r.k[0], r.stride[0]
    pd = kd // 2
    Do = (r.D + 2 * pd - kd) // sd + 1
    calls = []
    for b in range(r.B):
        for dz in [pd] + [t for t in range(kd) if t != pd]:
            hit = [(zo, zo * sd + dz - pd) for zo in range(Do) if 0 <= zo * sd + dz - pd < r.D]
            if hit:
                assert [zo for zo, _ in hit] == list(range(hit[0][0], hit[0][0] + len(hit)))
                calls.append((b, dz, hit[0][0], [zi for _, zi in hit]))
    return calls


# ---- transposed layers -----------------------------------------------------------------------------------------------------------------------
TRow = namedtuple("TRow", "n dims k B C Cout size bias")
T_ROWS = [
    TRow(1, 3, (2, 2, 2), 2, 40, 24, (3, 5, 7), False),
    TRow(2, 3, (1, 2, 2), 2, 40, 24, (3, 5, 7), True),
    TRow(3, 3, (2, 2, 2), 2, 40, 24, (1, 5, 7), True),       # the bias lands once per output voxel, not once per tap
    TRow(4, 2, (2, 1), 2, 40, 24, (5, 7), True),
    TRow(5, 2, (1, 2), 2, 40, 24, (5, 7), True),
]


def trow_id(r):
    return "T%d_k%s" % (r.n, "".join(map(str, r.k)))


@functools.lru_cache(maxsize=None)
def t_operands(r):
    seed = 9000 + 100 * r.n
    x = randn(r.B, r.C, *r.size, seed=seed)
    w = randn(r.C, r.Cout, *r.k, seed=seed + 1) / math.sqrt(r.C)          # every output voxel sums C products
    if r.n == 1:
        w[:, :, 1] *= 0.25              # one row whose taps are packed with different scale exponents
    return x, w, (randn(r.Cout, seed=seed + 2) if r.bias else None)


def t_host_scales(r, w):
    """as host_scales: one packing per depth tap of a ConvTranspose3d ([Cout * 4, Cin] GEMM rows), one for an anisotropic ConvTranspose2d"""
    from cineflow import ops
    gemm = lambda t: t.permute(1, 2, 3, 0).reshape(-1, t.shape[0], 1, 1)
    if r.dims == 2:
        return (ops.pack_conv_weight_f16s(gemm(w))[1],)
    return tuple(ops.pack_conv_weight_f16s(gemm(w[:, :, dz]))[1] for dz in range(r.k[0]))


def transposed_reference(x, w, b, scales):
    """fp64 {y3, y1, true, A, d3} of ConvTranspose{2,3}d(kernel = stride = w.shape[2:]): a 3-D layer has one scale per depth tap (each tap
    is its own packing), a 2-D layer has one.  Placement is F.conv_transpose{2,3}d's, on a weight that is zero outside the tap."""
    k = tuple(w.shape[2:])
    convt = (F.conv_transpose3d if len(k) == 3 else F.conv_transpose2d)
    conv = lambda a, m: convt(a, m, stride=k)
    ntap = k[0] if len(k) == 3 else 1
    assert len(scales) == ntap
    xh, xl = split_x(x)
    xa = xh.abs() + xl.abs()
    c = x.shape[1] - 1
    bb = (b.double() if b is not None else torch.zeros(w.shape[1], dtype=torch.float64)).view((1, -1) + (1,) * len(k))
    y3 = y1 = A = d3 = 0.0
    for dz in range(ntap):
        wh, wl = torch.zeros(w.shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64)
        if len(k) == 3:
            wh[:, :, dz], wl[:, :, dz] = split_w(w[:, :, dz], scales[dz])
        else:
            wh, wl = split_w(w, scales[0])
        sc = 2.0 ** -scales[dz]
        y3 = y3 + sc * _three(conv, xh, xl, wh, wl)
        y1 = y1 + sc * conv(xh, wh)
        A = A + sc * conv(xa, wh.abs() + wl.abs())
        d3 = d3 + sc * _three(conv, xh[:, c:], xl[:, c:], wh[c:], wl[c:])      # transposed weights: input channels on dim 0
    return dict(y3=y3 + bb, y1=y1 + bb, true=conv(x.double(), w.double()) + bb, A=A + bb.abs(), d3=d3)


@functools.lru_cache(maxsize=None)
def t_reference(r, scales):
    x, w, b = t_operands(r)
    return transposed_reference(x, w, b, scales)


def t_swaps(r, y):
    """{name: y with two interleaved output positions exchanged}: the depth taps of a (2,2,2) layer, the sub-rows / sub-columns of an
    anisotropic 2-D layer"""
    s = tuple(y.shape)
    if r.dims == 3:
        return {"depth taps": y.view(s[0], s[1], s[2] // 2, 2, s[3], s[4]).flip(3).reshape(s)} if r.k[0] == 2 else {}
    if r.k == (2, 1):
        return {"sub-rows": y.view(s[0], s[1], s[2] // 2, 2, s[3]).flip(3).reshape(s)}
    return {"sub-columns": y.view(s[0], s[1], s[2], s[3] // 2, 2).flip(4).reshape(s)}
