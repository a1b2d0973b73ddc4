"""Thin tensor-level wrappers over the C ABI (include/cineflow.h).

PyTorch is used for device memory (torch.empty on the caching allocator) and the current HIP stream only; every
number is produced by a hand-written HIP kernel in libcineflow_hip.so.  Inputs must be CUDA(=HIP) tensors; nothing
here runs on the CPU and nothing falls back to torch operators.
"""
import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from ._lib import lib, check

ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2, "lrelu": 3, "tanh": 4, "sigmoid": 5}
ACT_COEF = dict(ACT, mish=6)      # cf_coef_apply's codes: the fused epilogues' plus Mish
RES = {None: 0, "none": 0, "before_act": 1, "after_act": 2}
OP = {"add": 0, "sub": 1, "mul": 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/HIP tensor (cineflow has no CPU path)" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t.data_ptr()


def _u8(t, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
        raise TypeError("%s must be a contiguous CUDA uint8 tensor" % name)
    return t.data_ptr()


def _opt(t, name="tensor"):
    return None if t is None else _f32(t, name)


# ------------------------------------------------------------------------------------------------ warp family
def warp_bilinear(flow, src):
    """SpatialTransformer.forward: flow [B,2,H,W] / src [B,C,H,W], or the 3-D branch flow [B,3,D,H,W] / src [B,C,D,H,W]."""
    if src.dim() == 5:
        B, C, D, H, W = src.shape
        assert flow.shape == (B, 3, D, H, W), (flow.shape, src.shape)
        out = torch.empty_like(src)
        check(lib().cf_warp_trilinear_3d(_f32(flow), _f32(src), _f32(out), B, C, D, H, W, _stream()), "cf_warp_trilinear_3d")
        return out
    B, C, H, W = src.shape
    assert flow.shape == (B, 2, H, W), (flow.shape, src.shape)
    out = torch.empty_like(src)
    check(lib().cf_warp_bilinear_2d(_f32(flow), _f32(src), _f32(out), B, C, H, W, _stream()), "cf_warp_bilinear_2d")
    return out


def vecint(vec, nsteps=7):
    if vec.dim() == 5:   # 3-D fields: the same scaling and squaring, one warp launch per step
        assert vec.shape[1] == 3
        v = mul(vec, torch.full((1,), 1.0 / (2 ** nsteps), dtype=torch.float32, device=vec.device))
        for _ in range(nsteps):
            v = add(v, warp_bilinear(v, v))
        return v
    B, two, H, W = vec.shape
    assert two == 2
    out = torch.empty_like(vec)
    tmp = torch.empty_like(vec)
    check(lib().cf_vecint_2d(_f32(vec), _f32(out), _f32(tmp), B, H, W, nsteps, _stream()), "cf_vecint_2d")
    return out


def warp_labels(flow, labels, num_classes=4):
    """flow [T,B,2,H,W] float32; labels uint8 [B,H,W] -> uint8 [T,B,H,W]."""
    T, B, two, H, W = flow.shape
    assert two == 2 and labels.shape == (B, H, W)
    out = torch.empty((T, B, H, W), dtype=torch.uint8, device=flow.device)
    check(lib().cf_warp_labels_2d(_f32(flow), _u8(labels), _u8(out), T, B, num_classes, H, W, _stream()), "cf_warp_labels_2d")
    return out


def memory_input(x0, xt, cum):
    B, one, H, W = x0.shape
    assert one == 1 and xt.shape == x0.shape and cum.shape == (B, 2, H, W)
    out = torch.empty((B, 6, H, W), dtype=torch.float32, device=x0.device)
    check(lib().cf_memory_input(_f32(x0), _f32(xt), _f32(cum), _f32(out), B, H, W, _stream()), "cf_memory_input")
    return out


def jacobian_det(disp):
    """disp [B,2,H,W] float32 -> float64 [B,H,W]; or the 3-D case disp [B,3,D,H,W] -> float64 [B,D,H,W]."""
    if disp.dim() == 5:
        B, three, D, H, W = disp.shape
        assert three == 3
        out = torch.empty((B, D, H, W), dtype=torch.float64, device=disp.device)
        check(lib().cf_jacobian_det_3d(_f32(disp), out.data_ptr(), B, D, H, W, _stream()), "cf_jacobian_det_3d")
        return out
    B, two, H, W = disp.shape
    assert two == 2
    out = torch.empty((B, H, W), dtype=torch.float64, device=disp.device)
    check(lib().cf_jacobian_det_2d(_f32(disp), out.data_ptr(), B, H, W, _stream()), "cf_jacobian_det_2d")
    return out


# ------------------------------------------------------------------------------------------------ correlation
def corr_volume(cur, prev, radius=4, stride=1):
    B, C, H, W = cur.shape
    assert prev.shape == cur.shape
    out = torch.empty((B, (2 * radius + 1) ** 2, H, W), dtype=torch.float32, device=cur.device)
    check(lib().cf_corr_volume(_f32(cur), _f32(prev), _f32(out), B, C, H, W, radius, stride, _stream()), "cf_corr_volume")
    return out


def corr_volume_route(cur, prev, radius=4, stride=1):
    """the kernel corr_volume launches for these tensors: 0 generic, 1 persistent fp32 (corr_volume_p7_kernel), 2 f16 MFMA; launches nothing"""
    B, C, H, W = cur.shape
    assert prev.shape == cur.shape
    return lib().cf_corr_volume_route(_f32(cur), _f32(prev), C, H, W, radius, stride)


def pyramid_numel(B, H, W, levels):
    N = H * W
    return sum(B * N * (H >> l) * (W >> l) for l in range(levels))


def corr_pyramid(f1, f2, levels=4):
    B, C, H, W = f1.shape
    assert f2.shape == f1.shape
    pyr = torch.empty(pyramid_numel(B, H, W, levels), dtype=torch.float32, device=f1.device)
    check(lib().cf_corr_pyramid(_f32(f1), _f32(f2), _f32(pyr), B, C, H, W, levels, _stream()), "cf_corr_pyramid")
    return pyr


def corr_lookup(pyr, coords, levels=4, radius=4):
    B, two, H, W = coords.shape
    assert two == 2 and pyr.numel() == pyramid_numel(B, H, W, levels)
    out = torch.empty((B, levels * (2 * radius + 1) ** 2, H, W), dtype=torch.float32, device=coords.device)
    check(lib().cf_corr_lookup(_f32(pyr), _f32(coords), _f32(out), B, H, W, levels, radius, _stream()), "cf_corr_lookup")
    return out


def convex_upsample(flow, mask):
    B, C, h, w = flow.shape
    assert mask.shape == (B, 576, h, w)
    out = torch.empty((B, C, 8 * h, 8 * w), dtype=torch.float32, device=flow.device)
    check(lib().cf_convex_upsample(_f32(flow), _f32(mask), _f32(out), B, C, h, w, _stream()), "cf_convex_upsample")
    return out


# ------------------------------------------------------------------------------------------------ conv / norm / attention
def prep_conv_weight(w):
    """torch conv weight [Cout,Cin,KH,KW] -> Wt [Cin*KH*KW, Cout] (done once at model load)."""
    cout = w.shape[0]
    return w.reshape(cout, -1).t().contiguous()


# ---- f16 hi/lo-split convolution (conv_f16s.hip) ------------------------------------------------------------------
CONV_MODE = "f16s"   # "f16s": f16-MFMA 3-term split where supported, exact fp32 MFMA elsewhere;  "f32": fp32 MFMA only


def set_conv_mode(mode):
    global CONV_MODE
    assert mode in ("f16s", "f32")
    CONV_MODE = mode


@contextlib.contextmanager
def conv_terms(terms):
    """Product mode of the f16-MFMA convolutions launched from this thread inside the block (cf_conv_terms): 3 = hi/lo split (f32-class,
    the default), 1 = hi x hi only -- operands rounded to fp16, fp32 accumulation: the reference's fp16 autocast on the segmentation path
    (mixed_precision=True, neural_network.py:140-146).  The flow path never runs in mode 1 (SegFlowGaussian.py:2905-2909 forces it off)."""
    prev = lib().cf_conv_terms(int(terms))
    try:
        yield
    finally:
        lib().cf_conv_terms(prev)


def f16s_supported(kh, kw, stride, pad):
    """kernel shapes of conv_f16s.hip: 3x3 pad 1 and 1x1 pad 0 at stride 1 / 2; the separable 1x5 pad (0,2) / 5x1 pad (2,0) of RAFT's
    SepConvGRU at stride 1.  (The 7x7 convolution of the 2-channel flow in RAFT's motion encoder stays on the exact fp32 kernel by
    design: padding 2 channels to a 16-channel chunk would do 8x the work.)"""
    pad = tuple(pad)
    if stride in (1, 2) and ((kh, kw, pad) == (3, 3, (1, 1)) or (kh, kw, pad) == (1, 1, (0, 0))):
        return True
    return stride == 1 and ((kh, kw, pad) == (1, 5, (0, 2)) or (kh, kw, pad) == (5, 1, (2, 0)))


def f16s_chunk(kh, kw):
    """channels per LDS chunk of the kernel shape (16 for 3x3, 32 otherwise)"""
    return 16 if (kh, kw) == (3, 3) else 32


def f16s_dynamic_ok(x1, x2, kh, kw=None, out_sample_elems=None, out_hw=None):
    """Run-time limits of conv_f16s.hip (conv_f16s_supported): one sample of each input below 2 GiB (32-bit buffer offsets; larger BATCHES
    are split inside the library) and -- when the caller passes them -- one output sample (all `out_ctotal` channels of the destination
    buffer, x4 for the transposed convolution's scatter) below 1 GiB, 8 of them when an output image has <= 256 pixels (the epilogue's
    32-bit store offsets).  A cat[x1, x2] whose split is not a chunk multiple is handled by split-aware weight packing
    (pack_conv_weight_f16s(w, c1=...)), not by another kernel."""
    per = lambda t: 0 if t is None else (t.numel() // t.shape[0]) * 4
    if out_sample_elems is not None and out_sample_elems * 4 * (8 if (out_hw is not None and out_hw <= 256) else 1) >= 2 ** 30:
        return False
    return per(x1) < 2 ** 31 and per(x2) < 2 ** 31


def _scaled_split(wmat, ck, nmt, c1=None):
    """The part the weight packers share: wmat [Cout, Cin, nstep] -> (hi, lo, s, nchunk).  s = clamp(floor(log2(1024 / max|wmat|)), -24, 24)
    (0 for an all-zero weight); 2^s * wmat is rounded to fp32, its rows zero-padded to nmt * 32 and its channels to whole chunks of ck --
    with 0 < c1 < Cin and c1 % ck the first c1 channels are padded to whole chunks on their own and the others follow (cat[x1, x2]) --
    and split into hi = fp16(v), lo = fp16(v - hi), each [nmt * 32, nchunk * ck, nstep]."""
    cout, cin, nstep = wmat.shape
    wmax = float(wmat.abs().max())
    s = int(math.floor(math.log2(1024.0 / wmax))) if wmax > 0 else 0
    s = max(-24, min(24, s))
    ws = (wmat * (2.0 ** s)).to(torch.float32)
    split = c1 is not None and 0 < c1 < cin and c1 % ck
    c1p = (c1 + ck - 1) // ck * ck if split else 0
    nchunk = c1p // ck + (cin - c1 + ck - 1) // ck if split else (cin + ck - 1) // ck
    wp = torch.zeros((nmt * 32, nchunk * ck, nstep), dtype=torch.float32, device=wmat.device)
    if split:
        wp[:cout, :c1] = ws[:, :c1]
        wp[:cout, c1p:c1p + cin - c1] = ws[:, c1:]
    else:
        wp[:cout, :cin] = ws
    hi = wp.half()
    return hi, (wp - hi.float()).half(), s, nchunk


def pack_conv_weight_f16s(w, c1=None):
    """torch conv weight [Cout,Cin,KH,KW] (3x3, 1x1, 1x5, 5x1) -> (packed fp16 tensor, scale exponent s).

    Fragment order [m-tile][chunk][tap][kstep][part hi/lo][lane = h*32 + r][j]: value = 2^s * W[mt*32 + r][chunk*CK + kstep*16 + 8h + j][tap],
    CK = 16 (3x3) or 32; m-tiles padded to an even count when Cout > 32, channels padded to CK; the power of two
    2^s brings max|W| to ~2^10 so that the lo halves stay in fp16's normal range (exact scaling, undone through alpha).
    c1: the input is cat[x1 (c1 channels), x2]: x1's channels are padded to whole chunks (zero weights), x2's follow -- the kernel
    switches input pointers at a chunk boundary."""
    cout, cin, kh, kw = w.shape
    ntap = kh * kw
    ck = f16s_chunk(kh, kw)
    ks = ck // 16
    nmt = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    hi, lo, s, nchunk = _scaled_split(w.reshape(cout, cin, ntap), ck, nmt, c1)
    x = torch.stack([hi, lo])                                  # [part, co, ci, tap]
    x = x.view(2, nmt, 32, nchunk, ks, 2, 8, ntap)             # part, mt, r, chunk, ks, h, j, tap
    x = x.permute(1, 3, 7, 4, 0, 5, 2, 6).contiguous()        # mt, chunk, tap, ks, part, h, r, j
    return x.view(-1), s


# ---- row Winograd F(2,3) form of the same convolution (conv_wino.hip) ----------------------------------------------------
WINO = os.environ.get("CF_CONV_WINO", "1") != "0"         # 0: every layer stays on the direct kernels (A/B knob; the library reads it too)
_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))      # G of F(2,3): U = G g along kx


def wino_ok(B, C1, C2, H, W, cout, prenorm=False):
    """does cf_conv2d_wino take this 3x3 / stride 1 / pad 1 layer?  (Cout in whole 128-channel blocks or a last block >= 96, W % 16 == 0,
    H a multiple of the tile rows)"""
    return bool(WINO and CONV_MODE == "f16s" and lib().cf_conv2d_wino_ok(B, C1, C2, H, W, cout, 1 if prenorm else 0) == 1)


def wino_form(B, C1, C2, H, W, cout, prenorm=False):
    """the kernel form cf_conv2d_wino runs this layer on at the current route level: 0 (not taken), 2 / 4 (one tile per workgroup, NTW unit
    tiles per wave; 4 only under the forced level 4) or 8 (persistent)"""
    if not (WINO and CONV_MODE == "f16s"):
        return 0
    return int(lib().cf_conv2d_wino_form(B, C1, C2, H, W, cout, 1 if prenorm else 0))


def wino_mfma(B, C1, C2, H, W, cout, prenorm=0):
    """the MFMA shape of the kernel cf_conv2d_wino runs this layer on at the current route level: 16 (the persistent kernel's 16x16x32 form),
    32 (any other Winograd form) or 0 (not taken).  prenorm: 0 none, 1 deferred norm + LeakyReLU, 2 deferred norm + GELU"""
    if not (WINO and CONV_MODE == "f16s"):
        return 0
    return int(lib().cf_conv2d_wino_mfma(B, C1, C2, H, W, cout, int(prenorm)))


def pack_conv_weight_wino(w, c1=None):
    """torch conv weight [Cout,Cin,3,3] -> (packed fp16 tensor, scale exponent s) for cf_conv2d_wino.

    U[co][ci][ky][pos] = sum_kx G[pos][kx] w[co][ci][ky][kx] in fp64 (G = the F(2,3) kernel transform), scaled by 2^s (max|U| -> ~2^10),
    rounded to fp32 and split into fp16 hi / lo.  Fragment order [m-tile][chunk][step = ky * 4 + pos][part hi/lo][lane = h*32 + r][j]:
    value = 2^s * U[mt*32 + r][chunk*16 + 8h + j][ky][pos]; m-tiles padded to whole 128-channel blocks, channels to 16; c1 as in
    pack_conv_weight_f16s (cat[x1, x2] with x1's channels padded to whole chunks)."""
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    U = torch.einsum("pk,ocyk->ocyp", G, w.to(torch.float64)).reshape(cout, cin, 12)
    nmt = 4 * ((cout + 127) // 128)
    hi, lo, s, nchunk = _scaled_split(U, 16, nmt, c1)
    x = torch.stack([hi, lo])                                  # [part, co, ci, step]
    x = x.view(2, nmt, 32, nchunk, 2, 8, 12)                   # part, mt, r, chunk, h, j, step
    x = x.permute(1, 3, 6, 0, 4, 2, 5).contiguous()           # mt, chunk, step, part, h, r, j
    return x.view(-1), s


def conv2d_wino(x1, wpk, wscale, bias, cout, x2=None, act=None, res=None, out=None, out_coff=0, alpha=1.0, stats_groups=None):
    """cf_conv2d_wino: 3x3 / stride 1 / pad 1; arguments and returns as conv2d_f16s (wpk from pack_conv_weight_wino)."""
    B, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    if out is None:
        out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x1.device)
    assert out.shape[0] == B and out.shape[2] == H and out.shape[3] == W
    if res is not None:
        assert res.shape == (B, cout, H, W)
    assert wpk.dtype == torch.float16 and wpk.is_cuda
    if F16S_RANGE_CHECK:
        _range_check(x1, x2)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x1.device)
    check(lib().cf_conv2d_wino(_f32(x1), C1, _opt(x2), C2, wpk.data_ptr(), _opt(bias), _opt(res), _f32(out), out.shape[1], out_coff, B, H, W,
                               cout, ACT[act], float(alpha) * (2.0 ** -wscale), ws_ptr, ws_groups, _stream()), "cf_conv2d_wino")
    return (out, ws) if stats_groups else out


def conv2d_wino_prenorm(x, coef, slope, wpk, wscale, bias, cout, stats_groups=None):
    """cf_conv2d_wino_prenorm: as conv2d_f16s_prenorm on the Winograd kernel."""
    B, C, H, W = x.shape
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x.device)
    check(lib().cf_conv2d_wino_prenorm(_f32(x), C, _f32(coef), float(slope), wpk.data_ptr(), _opt(bias), _f32(out), B, H, W, cout, 2.0 ** -wscale,
                                       ws_ptr, ws_groups, _stream()), "cf_conv2d_wino_prenorm")
    return (out, ws) if stats_groups else out


# CF_F16S_RANGE_CHECK=1 (debug): every input of an f16-split convolution is scanned for values the hi/lo split cannot carry (non-finite or
# |x| >= 65504, e.g. a `noNorm` modality fed to a network without an input normalisation); f16s_range_violations() returns the count so far.
# Such values come out of the kernel as NaN by design; the exact route for them is set_conv_mode("f32").
F16S_RANGE_CHECK = os.environ.get("CF_F16S_RANGE_CHECK", "0") == "1"
_range_counter = {}


def _range_check(*tensors):
    for t in tensors:
        if t is None:
            continue
        c = _range_counter.get(t.device)
        if c is None:
            c = _range_counter[t.device] = torch.zeros(1, dtype=torch.int64, device=t.device)
        check(lib().cf_count_out_of_range(_f32(t), t.numel(), 65504.0, c.data_ptr(), _stream()), "cf_count_out_of_range")


def f16s_range_violations(reset=False):
    """number of f16-split convolution input elements seen outside the supported range since the last reset (0 unless F16S_RANGE_CHECK)"""
    n = sum(int(c.item()) for c in _range_counter.values())
    if reset:
        for c in _range_counter.values():
            c.zero_()
    return n


_zero_pool = {}


def _zeroed_stats_ws(n, device):
    """n doubles of a pool cleared with ONE memset (the convolution's fused GroupNorm statistics accumulate with atomics and need a
    zero start; a memset per launch was 1.2 % of the step).  Slices are handed out once; an exhausted pool is replaced by a fresh
    zeroed one (the old one lives as long as its slices do)."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    pool = _zero_pool.get(key)
    if pool is None or pool[1] + n > pool[0].numel():
        pool = [torch.zeros(max(n, 1 << 23), dtype=torch.float64, device=device), 0]   # 64 MB
        _zero_pool[key] = pool
    ws = pool[0][pool[1]:pool[1] + n]
    pool[1] += (n + 1) & ~1   # keep 16-byte alignment
    return ws


def _stats_args(stats_groups, B, device):
    """the statistics arguments of a convolution launch: (workspace or None, its pointer or None, the group count as the C ABI takes it --
    negative: the workspace is already zero, no memset in the library)"""
    if not stats_groups:
        return None, None, 0
    ws = _zeroed_stats_ws(2 * B * stats_groups, device)
    return ws, ws.data_ptr(), -stats_groups


def conv2d_f16s(x1, wpk, wscale, bias, cout, kh, kw, stride=1, pad=(0, 0), x2=None, act=None, res=None, out=None, out_coff=0, alpha=1.0,
                stats_groups=None):
    """With stats_groups=G the call returns (out, ws): ws holds the GroupNorm statistics of `out` for group_norm_apply."""
    B, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    Ho = (H + 2 * pad[0] - kh) // stride + 1
    Wo = (W + 2 * pad[1] - kw) // stride + 1
    if out is None:
        out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x1.device)
    assert out.shape[0] == B and out.shape[2] == Ho and out.shape[3] == Wo
    if res is not None:
        assert res.shape == (B, cout, Ho, Wo)
    assert wpk.dtype == torch.float16 and wpk.is_cuda
    if F16S_RANGE_CHECK:
        _range_check(x1, x2)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x1.device)
    check(lib().cf_conv2d_f16s(_f32(x1), C1, _opt(x2), C2, wpk.data_ptr(), _opt(bias), _opt(res), _f32(out), out.shape[1], out_coff, B, H, W,
                               cout, kh, kw, stride, pad[0], pad[1], ACT[act], float(alpha) * (2.0 ** -wscale),
                               ws_ptr, ws_groups, _stream()), "cf_conv2d_f16s")
    return (out, ws) if stats_groups else out


F16sRoute = collections.namedtuple("F16sRoute", "route tup terms nimg fused part")


def conv2d_f16s_route(x1, cout, kh, kw, stride=1, pad=(0, 0), x2=None, prenorm=False, transposed=False, stats_groups=None):
    """The plan conv2d_f16s (conv2d_f16s_prenorm with prenorm=True, conv_transpose2d_k2s2_f16s with transposed=True) executes for a plain
    call on these tensors in the current conv_terms mode (cf_conv2d_f16s_route; host code, launches nothing): route 0 declined / 1
    conv_f16s_kernel / 2 conv_stream_kernel, tup = the instantiation <KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL> (route 1), TERMS, images
    per workgroup, whether the epilogue accumulates the statistics, samples per launch."""
    B, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    plan = (ctypes.c_int * 15)()
    route = lib().cf_conv2d_f16s_route(B, C1, C2, H, W, cout, kh, kw, stride, pad[0], pad[1], x1.data_ptr() & 15,
                                       0 if x2 is None else x2.data_ptr() & 15, int(prenorm), int(transposed), stats_groups or 0, plan)
    check(min(route, 0), "cf_conv2d_f16s_route")
    return F16sRoute(route, tuple(plan[1:11]), plan[11], plan[12], bool(plan[13]), plan[14])


# ---- 3-D convolution (conv3d_f16s.hip) -----------------------------------------------------------------------------------
def pack_conv3d_weight_f16s(w, c1=None):
    """torch Conv3d weight [Cout,Cin,KD,3,3] -> (packed fp16 tensor, scale exponent s) for cf_conv3d_f16s: pack_conv_weight_f16s' fragment
    order with the KD * 9 taps in (dz, ky, kx) order, 16-channel chunks; c1 as there (cat[x1, x2] with x1 padded to whole chunks)."""
    cout, cin, kd, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and kd in (1, 3)
    ntap = kd * 9
    nmt = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    hi, lo, s, nchunk = _scaled_split(w.reshape(cout, cin, ntap), 16, nmt, c1)
    x = torch.stack([hi, lo]).view(2, nmt, 32, nchunk, 2, 8, ntap)      # part, mt, r, chunk, h, j, tap
    return x.permute(1, 3, 6, 0, 4, 2, 5).contiguous().view(-1), s     # mt, chunk, tap, part, h, r, j


def conv3d_f16s_ok(B, C1, C2, D, H, W, cout, kernel, stride):
    """does cf_conv3d_f16s take this layer?  kernel (1|3,3,3), stride (1|2, s, s) with s in {1,2}, every sample < 2 GiB, three-term mode."""
    kernel, stride = tuple(kernel), tuple(stride)
    if kernel[1] != kernel[2] or stride[1] != stride[2]:
        return False
    return lib().cf_conv3d_f16s_ok(B, C1, C2, D, H, W, cout, kernel[0], kernel[1], stride[0], stride[1]) == 1


def conv3d_f16s(x1, wpk, wscale, bias, cout, kernel, stride=(1, 1, 1), x2=None, out=None, alpha=1.0, stats_groups=None):
    """cf_conv3d_f16s on NCDHW tensors, padding (kd // 2, 1, 1).  With stats_groups=G the call returns (out, ws): ws holds the GroupNorm /
    InstanceNorm statistics of `out` over (D, H, W) for group_norm_apply."""
    B, C1, D, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    kd, kh, kw = kernel
    sd, st = stride[0], stride[1]
    assert stride[1] == stride[2]
    if x2 is not None:
        assert x2.shape[0] == B and tuple(x2.shape[2:]) == (D, H, W)
    shape = (B, cout, (D + 2 * (kd // 2) - kd) // sd + 1, (H - 1) // st + 1, (W - 1) // st + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x1.device)
    assert tuple(out.shape) == shape
    assert wpk.dtype == torch.float16 and wpk.is_cuda
    if F16S_RANGE_CHECK:
        _range_check(x1, x2)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x1.device)
    check(lib().cf_conv3d_f16s(_f32(x1), C1, _opt(x2), C2, wpk.data_ptr(), _opt(bias), _f32(out), B, D, H, W, cout, kd, kh, kw, sd, st,
                               float(alpha) * (2.0 ** -wscale), ws_ptr, ws_groups,
                               _stream()), "cf_conv3d_f16s")
    return (out, ws) if stats_groups else out


# ---- strided (1,1,1) 3-D convolution (conv3d_pw_f16s.hip) -------------------------------------------------------------------
def pack_conv3d_pw_weight_f16s(w):
    """torch Conv3d weight [Cout,Cin,1,1,1] -> (packed fp16 tensor, scale exponent s) for cf_conv3d_pw_f16s: pack_conv_weight_f16s' 1x1
    fragment order (32-channel chunks of two k-steps)."""
    cout, cin = w.shape[:2]
    assert tuple(w.shape[2:]) == (1, 1, 1)
    return pack_conv_weight_f16s(w.reshape(cout, cin, 1, 1))


def conv3d_pw_f16s_ok(B, Cin, D, H, W, cout, stride):
    """does cf_conv3d_pw_f16s take this layer?  stride (1|2, s, s) with s in {1,2}, every sample < 2 GiB, three-term mode."""
    stride = tuple(stride)
    if stride[1] != stride[2]:
        return False
    return lib().cf_conv3d_pw_f16s_ok(B, Cin, D, H, W, cout, stride[0], stride[1]) == 1


def conv3d_pw_f16s(x, wpk, wscale, bias, cout, stride, out=None, alpha=1.0, stats_groups=None):
    """cf_conv3d_pw_f16s on NCDHW tensors: the (1,1,1) convolution at stride (sd, s, s), no padding.  With stats_groups=G the call returns
    (out, ws): ws holds the GroupNorm / InstanceNorm statistics of `out` over (D, H, W) for group_norm_apply."""
    B, Cin, D, H, W = x.shape
    sd, st = stride[0], stride[1]
    assert stride[1] == stride[2]
    shape = (B, cout, (D - 1) // sd + 1, (H - 1) // st + 1, (W - 1) // st + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == shape
    assert wpk.dtype == torch.float16 and wpk.is_cuda
    nmt = 1 if cout <= 32 else 2 * ((cout + 63) // 64)
    assert wpk.numel() == nmt * 32 * ((Cin + 31) // 32) * 32 * 2, "wpk is not pack_conv3d_pw_weight_f16s of a [%d, %d, 1, 1, 1] weight" % (cout, Cin)
    assert bias is None or tuple(bias.shape) == (cout,)
    if F16S_RANGE_CHECK:
        _range_check(x)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x.device)
    check(lib().cf_conv3d_pw_f16s(_f32(x), wpk.data_ptr(), _opt(bias), _f32(out), B, Cin, D, H, W, cout, sd, st,
                                  float(alpha) * (2.0 ** -wscale), ws_ptr, ws_groups, _stream()), "cf_conv3d_pw_f16s")
    return (out, ws) if stats_groups else out


def small_cin_supported(cin, kh, kw, stride, pad, stats_groups=None):
    """layers routed to cf_conv2d_small_cin: 1 or 2 input channels (3x3 pad 1 or 1x1) and 6 input channels 1x1, stride 1, <= 64
    statistics groups.  Measured at 256x256 (tools/microbench.py --only stem): 1 -> 32 B120 209 us vs 641 us on the MFMA kernel,
    1 -> 64 106 vs 238, 6 -> 64 1x1 120 vs 194; the 6 -> 64 3x3 layer is FMA-bound in the direct kernel (304 vs 257 us) and stays
    on the MFMA kernel."""
    if stride != 1 or (stats_groups and stats_groups > 64):
        return False
    k3, k1 = (kh, kw, tuple(pad)) == (3, 3, (1, 1)), (kh, kw, tuple(pad)) == (1, 1, (0, 0))
    return (cin in (1, 2) and (k3 or k1)) or (cin == 6 and k1)


def conv2d_small_cin(x, weight, bias, stats_groups=None):
    """Stem convolution as a direct fp32 kernel: x [B,Cin,H,W], weight [Cout,Cin,K,K] (checkpoint layout).  With stats_groups=G the
    call returns (out, ws) like conv2d_f16s."""
    B, Cin, H, W = x.shape
    cout, cin_w, K, K2 = weight.shape
    assert cin_w == Cin and K == K2
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    ws = torch.empty(2 * B * stats_groups, dtype=torch.float64, device=x.device) if stats_groups else None
    check(lib().cf_conv2d_small_cin(_f32(x), _f32(weight), _opt(bias), _f32(out), B, Cin, H, W, cout, K, None if ws is None else ws.data_ptr(),
                                    stats_groups or 0, _stream()), "cf_conv2d_small_cin")
    return (out, ws) if stats_groups else out


def small_cout_supported(cout, kh, kw, stride, pad):
    """layers routed to cf_conv2d_small_cout: 3x3 / pad 1 / stride 1 with at most 4 output channels (the flow heads).  Measured at
    128 x 64 x 256 x 256 -> 2: see DESIGN.md (the MFMA kernel fills 2 of its 32 rows: 16 TF)."""
    return cout <= 4 and (kh, kw, tuple(pad)) == (3, 3, (1, 1)) and stride == 1


def conv2d_small_cout(x, weight, bias, res=None):
    """Direct exact-fp32 3x3 convolution to <= 4 channels: x [B,Cin,H,W], weight [Cout,Cin,3,3] (checkpoint layout) -> conv + bias (+ res)."""
    B, Cin, H, W = x.shape
    cout = weight.shape[0]
    assert tuple(weight.shape) == (cout, Cin, 3, 3)
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.shape == out.shape
    check(lib().cf_conv2d_small_cout(_f32(x), _f32(weight), _opt(bias), _opt(res), _f32(out), B, Cin, H, W, cout, _stream()), "cf_conv2d_small_cout")
    return out


def small_cout_norm2_ok(y2, cout, kh, kw, stride, pad):
    """can cf_conv2d_small_cout_norm2 take the raw block outputs y2 (and r, same shape) into a `cout`-channel 3x3 head?"""
    B, C, H, W = y2.shape
    return bool(CONV_MODE == "f16s" and small_cout_supported(cout, kh, kw, stride, pad) and lib().cf_conv2d_small_cout_norm2_ok(B, C, H, W, cout) == 1)


def conv2d_small_cout_norm2(y2, coef2, r, coefr, weight, bias):
    """conv2d_small_cout of GELU(GN2(y2)) + GN_ds(r) -- a DoubleConv's output -- from the block's raw maps y2, r [B,Cin,H,W] and their
    group_norm_coef tables [B,3,Cin]: the block's final apply pass happens while the head stages its input."""
    B, Cin, H, W = y2.shape
    cout = weight.shape[0]
    assert tuple(weight.shape) == (cout, Cin, 3, 3) and r.shape == y2.shape
    assert tuple(coef2.shape) == (B, 3, Cin) and tuple(coefr.shape) == (B, 3, Cin)
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=y2.device)
    check(lib().cf_conv2d_small_cout_norm2(_f32(y2), _f32(coef2), _f32(r), _f32(coefr), _f32(weight), _opt(bias), _f32(out), B, Cin, H, W, cout,
                                           _stream()), "cf_conv2d_small_cout_norm2")
    return out


def stem_block_ok(x, cout, groups):
    """can cf_stem_block take x [B,Cin,H,W] (Cin 1 or 6) into the `cout`-channel 3x3 and 1x1 maps with `groups` statistics groups?"""
    B, Cin, H, W = x.shape
    return bool(CONV_MODE == "f16s" and lib().cf_stem_block_ok(B, Cin, H, W, cout, groups) == 1)


def stem_block(x, w3, b3, w1, b1, groups):
    """conv1 (3x3 pad 1) and the 1x1 downsample convolution of a stem DoubleConv in one launch over x: -> (y, ws_y, r, ws_r), the two raw
    maps [B,Cout,H,W] with the GroupNorm statistics of each (as conv2d_small_cin returns them)."""
    B, Cin, H, W = x.shape
    cout = w3.shape[0]
    assert tuple(w3.shape) == (cout, Cin, 3, 3) and tuple(w1.shape) == (cout, Cin, 1, 1)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    r = torch.empty_like(y)
    ws = _zeroed_stats_ws(4 * B * groups, x.device)
    ws_y, ws_r = ws[:2 * B * groups], ws[2 * B * groups:]
    check(lib().cf_stem_block(_f32(x), _f32(w3), _opt(b3), _f32(w1), _opt(b1), _f32(y), _f32(r), B, Cin, H, W, cout, ws_y.data_ptr(), ws_r.data_ptr(),
                              -groups, _stream()), "cf_stem_block")
    return y, ws_y, r, ws_r


def stem_block_y(x, w3, b3, w1, b1, groups):
    """stem_block without the shortcut map: -> (y, ws_y, ws_r).  r = conv1x1(x; w1, b1) is summed into ws_r but never stored; the block's
    final pass rebuilds it from x (group_norm_apply_res_stem)."""
    B, Cin, H, W = x.shape
    cout = w3.shape[0]
    assert tuple(w3.shape) == (cout, Cin, 3, 3) and tuple(w1.shape) == (cout, Cin, 1, 1)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    ws = _zeroed_stats_ws(4 * B * groups, x.device)
    ws_y, ws_r = ws[:2 * B * groups], ws[2 * B * groups:]
    check(lib().cf_stem_block_y(_f32(x), _f32(w3), _opt(b3), _f32(w1), _opt(b1), _f32(y), B, Cin, H, W, cout, ws_y.data_ptr(), ws_r.data_ptr(), -groups,
                                _stream()), "cf_stem_block_y")
    return y, ws_y, ws_r


def group_norm_apply_res_stem_ok(x, c, groups):
    """can cf_group_norm_apply_res_stem rebuild a `c`-channel 1x1 shortcut of x [B,Cin,H,W] inside the apply pass?"""
    B, Cin, H, W = x.shape
    return bool(CONV_MODE == "f16s" and x.data_ptr() % 16 == 0 and lib().cf_group_norm_apply_res_stem_ok(B, Cin, c, H, W, groups) == 1)


def group_norm_apply_res_stem(y2, gamma, beta, groups, ws, x, w1, b1, ws_r, gamma_r, beta_r, eps=1e-5, act=None, res_mode="after_act", out=None):
    """group_norm_apply(y2, ..., res=r, res_norm=(ws_r, gamma_r, beta_r)) with r = conv1x1(x; w1, b1) rebuilt inside the pass instead of
    read: the same bits as that call on the r stem_block stores."""
    B, C, H, W = y2.shape
    Cin = x.shape[1]
    assert tuple(x.shape) == (B, Cin, H, W) and tuple(w1.shape) == (C, Cin, 1, 1) and res_mode in ("before_act", "after_act")
    assert ws.dtype == torch.float64 and ws.numel() >= 2 * B * groups and ws_r.dtype == torch.float64 and ws_r.numel() >= 2 * B * groups
    if out is None:
        out = torch.empty_like(y2)
    check(lib().cf_group_norm_apply_res_stem(_f32(y2), _opt(gamma), _opt(beta), ws.data_ptr(), _f32(x), _f32(w1), _opt(b1), ws_r.data_ptr(),
                                             _opt(gamma_r), _opt(beta_r), _f32(out), B, Cin, C, H, W, groups, float(eps), ACT[act], RES[res_mode],
                                             _stream()), "cf_group_norm_apply_res_stem")
    return out


def prenorm_ok(x, cout):
    """can cf_conv2d_f16s_prenorm take this input (raw conv output [B,C,H,W]) for a 3x3 / stride 1 convolution to `cout` channels?"""
    B, C, H, W = x.shape
    return bool(CONV_MODE == "f16s" and x.data_ptr() % 16 == 0 and lib().cf_conv2d_f16s_prenorm_ok(B, C, H, W, cout) == 1)


def group_norm_coef(ws, gamma, beta, groups, B, C, HW, eps=1e-5):
    """{mean, rstd * gamma, beta} per (sample, channel) from a statistics workspace -> float [B,3,C] for conv2d_f16s_prenorm"""
    coef = torch.empty((B, 3, C), dtype=torch.float32, device=ws.device)
    check(lib().cf_group_norm_coef(ws.data_ptr(), _opt(gamma), _opt(beta), B, C, HW, groups, float(eps), _f32(coef), _stream()), "cf_group_norm_coef")
    return coef


def batch_norm_coef(running_mean, running_var, gamma, beta, B, eps=1e-5):
    """BatchNorm in eval mode as a table: float [B,3,C] = {running_mean, gamma / sqrt(running_var + eps), beta}, group_norm_coef's layout"""
    C = running_mean.numel()
    coef = torch.empty((B, 3, C), dtype=torch.float32, device=running_mean.device)
    check(lib().cf_batch_norm_coef(_f32(running_mean), _f32(running_var), _opt(gamma), _opt(beta), float(eps), B, C, _f32(coef), _stream()),
          "cf_batch_norm_coef")
    return coef


def coef_apply_ok(B, C, HW):
    """does cf_coef_apply's index arithmetic hold [B, C, HW]?"""
    return lib().cf_coef_apply_ok(int(B), int(C), int(HW)) == 1


def coef_apply(x, coef=None, act=None, slope=0.01, out=None):
    """out = act((x - mean) * scale + shift) with coef [B,3,C] = {mean, scale, shift} (group_norm_coef / batch_norm_coef); coef None: the
    activation alone.  act: an ACT_COEF name ('mish' included); 'lrelu' takes `slope`.  x [B,C,...] (an NCDHW tensor as its rows);
    out may be x or a tensor of x's shape -- contiguous, but at any 4-byte address (a view into a larger buffer)."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and (coef is None or tuple(coef.shape) == (B, 3, C))
    check(lib().cf_coef_apply(_f32(x), _opt(coef), ACT_COEF[act], float(slope), _f32(out), B, C, HW, _stream()), "cf_coef_apply")
    return out


def norm_head_ok(x, K):
    """can cf_norm_head_1x1 take the raw map x [B,C,H,W] into K classes?"""
    return x.dim() == 4 and K in (2, 4, 8) and (x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[1] <= 1024 and x.is_contiguous()


def norm_head_1x1(x, coef, slope, w, bias=None):
    """out[b,k] = bias[k] + sum_c w[k,c] * lrelu((x[b,c] - mean) * scale + shift, slope): the deferred InstanceNorm + LeakyReLU of a raw
    convolution output x [B,C,H,W] (coef from group_norm_coef) folded into a 1x1 head w [K,C] (Generic_UNet's seg_outputs[-1])."""
    B, C, H, W = x.shape
    K = w.shape[0]
    w2 = w.reshape(K, C).contiguous()
    out = torch.empty((B, K, H, W), dtype=torch.float32, device=x.device)
    check(lib().cf_norm_head_1x1(_f32(x), _f32(coef), float(slope), _f32(w2), _opt(bias), _f32(out), B, C, H * W, K, _stream()), "cf_norm_head_1x1")
    return out


def conv2d_f16s_prenorm(x, coef, slope, wpk, wscale, bias, cout, stats_groups=None):
    """3x3 / stride 1 convolution of lrelu((x - mean) * scale + shift, slope): x is the producer's raw output, coef its
    group_norm_coef.  Returns (out, ws) with stats_groups like conv2d_f16s."""
    B, C, H, W = x.shape
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x.device)
    check(lib().cf_conv2d_f16s_prenorm(_f32(x), C, _f32(coef), float(slope), wpk.data_ptr(), _opt(bias), _f32(out), B, H, W, cout, 2.0 ** -wscale,
                                       ws_ptr, ws_groups, _stream()), "cf_conv2d_f16s_prenorm")
    return (out, ws) if stats_groups else out


def conv_transpose2d_k2s2_f16s(x, wpk, wscale, bias, cout, out=None, out_coff=0, stats_groups=None):
    B, Cin, H, W = x.shape
    if F16S_RANGE_CHECK:
        _range_check(x)
    if out is None:
        out = torch.empty((B, cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    ws, ws_ptr, ws_groups = _stats_args(stats_groups, B, x.device)       # fused into the scatter epilogue (atomics: zero start)
    check(lib().cf_conv_transpose2d_k2s2_f16s(_f32(x), wpk.data_ptr(), _opt(bias), _f32(out), out.shape[1], out_coff, B, Cin, H, W, cout,
                                              2.0 ** -wscale, ws_ptr, ws_groups, _stream()),
          "cf_conv_transpose2d_k2s2_f16s")
    return (out, ws) if stats_groups else out


def conv2d(x1, wt, bias, cout, kh, kw, stride=1, pad=(0, 0), x2=None, act=None, res=None, out=None, out_coff=0, alpha=1.0,
           w_bstride=0):
    """act(alpha*conv(cat[x1,x2]) + bias) + res, written into channels [out_coff, out_coff+cout) of `out`."""
    B, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    if x2 is not None:
        assert x2.shape[0] == B and x2.shape[2:] == x1.shape[2:]
    assert wt.shape == ((C1 + C2) * kh * kw, cout) or w_bstride, (wt.shape, C1, C2, kh, kw, cout)
    Ho = (H + 2 * pad[0] - kh) // stride + 1
    Wo = (W + 2 * pad[1] - kw) // stride + 1
    if out is None:
        out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x1.device)
    assert out.shape[0] == B and out.shape[2] == Ho and out.shape[3] == Wo
    if res is not None:
        assert res.shape == (B, cout, Ho, Wo)
    check(lib().cf_conv2d(_f32(x1), C1, _opt(x2), C2, _f32(wt), w_bstride, _opt(bias), _opt(res), _f32(out), out.shape[1], out_coff,
                          B, H, W, cout, kh, kw, stride, pad[0], pad[1], ACT[act], float(alpha), _stream()), "cf_conv2d")
    return out


def conv_transpose2d_k2s2(x, w, bias, out=None, out_coff=0):
    """w in torch layout [Cin,Cout,2,2]."""
    B, Cin, H, W = x.shape
    assert w.shape[0] == Cin and w.shape[2:] == (2, 2)
    cout = w.shape[1]
    if out is None:
        out = torch.empty((B, cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    check(lib().cf_conv_transpose2d_k2s2(_f32(x), _f32(w), _opt(bias), _f32(out), out.shape[1], out_coff, B, Cin, H, W, cout,
                                         _stream()), "cf_conv_transpose2d_k2s2")
    return out


_ws_cache = {}


def _stats_ws(n, device):
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(max(n, 4096), dtype=torch.float64, device=device)
        _ws_cache[key] = ws
    return ws


def group_norm(x, gamma, beta, groups, eps=1e-5, act=None, res=None, res_mode=None, out=None):
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    if out is None:
        out = torch.empty_like(x)
    ws = _stats_ws(2 * B * groups, x.device)
    check(lib().cf_group_norm(_f32(x), _opt(gamma), _opt(beta), _opt(res), _f32(out), B, C, HW, groups, float(eps), ACT[act],
                              RES[res_mode if res is not None else None], ws.data_ptr(), _stream()), "cf_group_norm")
    return out


def group_norm_apply(x, gamma, beta, groups, ws, eps=1e-5, act=None, res=None, res_mode=None, out=None, res_norm=None):
    """Apply pass only; `ws` from conv2d_f16s(..., stats_groups=groups).  res_norm=(ws_r, gamma_r, beta_r): `res` is a raw
    convolution output whose own GroupNorm (same groups / eps) is applied on the fly while it is added."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    if out is None:
        out = torch.empty_like(x)
    assert ws.dtype == torch.float64 and ws.numel() >= 2 * B * groups
    if res_norm is not None:
        ws_r, gamma_r, beta_r = res_norm
        assert res is not None and res_mode in ("before_act", "after_act") and res.shape == x.shape
        assert ws_r.dtype == torch.float64 and ws_r.numel() >= 2 * B * groups
        check(lib().cf_group_norm_apply_res_norm(_f32(x), _opt(gamma), _opt(beta), _f32(res), _f32(out), B, C, HW, groups, float(eps), ACT[act],
                                                 RES[res_mode], ws.data_ptr(), ws_r.data_ptr(), _opt(gamma_r), _opt(beta_r), _stream()),
              "cf_group_norm_apply_res_norm")
        return out
    check(lib().cf_group_norm_apply(_f32(x), _opt(gamma), _opt(beta), _opt(res), _f32(out), B, C, HW, groups, float(eps), ACT[act],
                                    RES[res_mode if res is not None else None], ws.data_ptr(), _stream()), "cf_group_norm_apply")
    return out


def group_norm_stats(x, groups):
    """The statistics pass of group_norm alone -> a fresh fp64 workspace [B, groups, 2] of {sum, sum of squares} per slab."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    ws = torch.empty((B, groups, 2), dtype=torch.float64, device=x.device)
    check(lib().cf_group_norm_stats(_f32(x), ws.data_ptr(), B, C, HW, groups, _stream()), "cf_group_norm_stats")
    return ws


GroupNormRoute = collections.namedtuple("GroupNormRoute", "stats_block segs stats_blocks apply_large vec ppb apply_blocks last_np")


def group_norm_route(x, out=None, res=None, groups=1):
    """The plan group_norm / group_norm_apply execute for these tensors (out None: a fresh, aligned tensor); launches nothing.
    stats_block: 0 gn_stats_wave_kernel, 1 gn_stats_block_kernel (segs blocks per slab); apply_large: 0 gn_apply_small_kernel (ppb planes
    per block, last_np in the last), 1 gn_apply_kernel (ppb blocks per plane); vec: the float4 instantiation."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    plan = (ctypes.c_int * 8)()
    check(lib().cf_group_norm_route(_f32(x), _opt(out), _opt(res), B, C, HW, groups, ctypes.addressof(plan)), "cf_group_norm_route")
    return GroupNormRoute(*plan)


def layer_norm_cf(x, gamma, beta, eps=1e-5, out=None):
    B, C, N = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().cf_layer_norm_cf(_f32(x), _f32(gamma), _f32(beta), _f32(out), B, C, N, float(eps), _stream()), "cf_layer_norm_cf")
    return out


def _cf_slice(t, name):
    """[B,C,N] tensor that is either contiguous or a channel slice (narrow on dim 1) of a contiguous buffer."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError("%s must be a 3-D CUDA float32 tensor" % name)
    B, C, N = t.shape
    if t.stride(2) != 1 or t.stride(1) != N:
        raise ValueError("%s must be contiguous in its last two dims" % name)
    return t.data_ptr(), (t.stride(0) if B > 1 else max(t.stride(0), C * N))


def attention_cf(q, k, v, heads):
    """q [B,C,Nq], k/v [B,C,Nk] channel-first; each may be a channel slice of a fused projection buffer.  Token counts that are not
    multiples of 32 (e.g. the 28 x 28 bottleneck of a 224 x 224 image) are zero-padded here and the padded keys masked in the kernel."""
    B, C, Nq = q.shape
    Nk = k.shape[2]
    assert k.shape == (B, C, Nk) and v.shape == (B, C, Nk) and C % heads == 0
    if Nq % 32 or Nk % 32:
        Nqp, Nkp = (Nq + 31) // 32 * 32, (Nk + 31) // 32 * 32

        def padded(t, n):
            p = torch.zeros((B, C, n), dtype=torch.float32, device=t.device)
            p[:, :, :t.shape[2]] = t
            return p
        qp_, kp_, vp_ = padded(q, Nqp), padded(k, Nkp), padded(v, Nkp)
        out = torch.empty((B, C, Nqp), dtype=torch.float32, device=q.device)
        check(lib().cf_attention_cf_masked(_f32(qp_), C * Nqp, _f32(kp_), C * Nkp, _f32(vp_), C * Nkp, _f32(out), B, heads, C // heads, Nqp, Nkp, Nk,
                                           _stream()), "cf_attention_cf_masked")
        return out[:, :, :Nq].contiguous()
    qp, qbs = _cf_slice(q, "q")
    kp, kbs = _cf_slice(k, "k")
    vp, vbs = _cf_slice(v, "v")
    out = torch.empty((B, C, Nq), dtype=torch.float32, device=q.device)
    check(lib().cf_attention_cf(qp, qbs, kp, kbs, vp, vbs, _f32(out), B, heads, C // heads, Nq, Nk, _stream()), "cf_attention_cf")
    return out


def attention_route(v, heads, Nq=None):
    """the kernel attention_cf launches for this v [B,C,Nk] (Nq: the query count of the call, when it is known): 0 attention_cf_kernel<d>
    (fp32 MFMA), 1 attention_cf_f16s_kernel<d> (f16 hi/lo split); launches nothing.  A ragged call (Nk or Nq not a multiple of 32) runs on
    attention_cf's zero-padded copy of v -- a fresh contiguous buffer of Nk rounded up to 32 --, so there only the head dimension decides."""
    B, C, Nk = v.shape
    assert C % heads == 0
    if Nk % 32 or (Nq is not None and Nq % 32):
        vp, vbs, Nk = 0, C * ((Nk + 31) // 32 * 32), (Nk + 31) // 32 * 32
    else:
        vp, vbs = _cf_slice(v, "v")
    r = lib().cf_attention_cf_route(vp, vbs, C // heads, Nk)
    if r < 0:
        check(r, "cf_attention_cf_route")
    return r


# ------------------------------------------------------------------------------------------------ plumbing kernels
def gru_reset_mul(gates, h):
    B, C = h.shape[0], h.shape[1]
    HW = h.numel() // (B * C)
    out = torch.empty_like(h)
    check(lib().cf_gru_reset_mul(_f32(gates), _f32(h), _f32(out), B, C, HW, _stream()), "cf_gru_reset_mul")
    return out


def gru_blend(gates, h, cand):
    B, C = h.shape[0], h.shape[1]
    HW = h.numel() // (B * C)
    out = torch.empty_like(h)
    check(lib().cf_gru_blend(_f32(gates), _f32(h), _f32(cand), _f32(out), B, C, HW, _stream()), "cf_gru_blend")
    return out


def binary(op, a, b, out=None):
    """a op b with b broadcast over the leading dims of a (b.numel() divides a.numel())."""
    n, period = a.numel(), b.numel()
    assert n % period == 0
    if out is None:
        out = torch.empty_like(a)
    check(lib().cf_binary(OP[op], _f32(a), _f32(b), _f32(out), n, period, _stream()), "cf_binary")
    return out


def add(a, b, out=None):
    return binary("add", a, b, out)


def sub(a, b, out=None):
    return binary("sub", a, b, out)


def mul(a, b, out=None):
    return binary("mul", a, b, out)


def copy_channels(src, src_coff, C, dst=None, dst_coff=0, act=None):
    B, sct = src.shape[0], src.shape[1]
    HW = src.numel() // (B * sct)
    if dst is None:
        dst = torch.empty((B, C) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
    check(lib().cf_copy_channels(_f32(src), sct, src_coff, _f32(dst), dst.shape[1], dst_coff, B, C, HW, ACT[act], _stream()),
          "cf_copy_channels")
    return dst


def coords_grid(B, H, W, device):
    out = torch.empty((B, 2, H, W), dtype=torch.float32, device=device)
    check(lib().cf_coords_grid(_f32(out), B, H, W, _stream()), "cf_coords_grid")
    return out


def crop2d(src, y0, x0, h, w):
    lead, (H, W) = src.shape[:-2], src.shape[-2:]
    N = src.numel() // (H * W)
    dst = torch.empty(tuple(lead) + (h, w), dtype=torch.float32, device=src.device)
    check(lib().cf_crop2d(_f32(src), _f32(dst), N, H, W, y0, x0, h, w, _stream()), "cf_crop2d")
    return dst


def pad2d(src, y0, x0, H, W):
    lead, (h, w) = src.shape[:-2], src.shape[-2:]
    N = src.numel() // (h * w)
    dst = torch.empty(tuple(lead) + (H, W), dtype=torch.float32, device=src.device)
    check(lib().cf_pad2d(_f32(src), _f32(dst), N, h, w, y0, x0, H, W, _stream()), "cf_pad2d")
    return dst


NONLIN_CODES = {"softmax": 0, "sigmoid": 1}     # CF_NONLIN_* of include/cineflow.h


def _nonlin_code(nonlin):
    if nonlin not in NONLIN_CODES:
        raise ValueError("nonlin must be 'softmax' or 'sigmoid', got %r" % (nonlin,))
    return NONLIN_CODES[nonlin]


def tta_accumulate(logits, acc, flip_h, flip_w, weight, nonlin="softmax"):
    """acc += weight * flip(nonlin(logits)); nonlin "softmax" over K (the default, cf_tta_accumulate) or "sigmoid" per channel (region heads)."""
    B, K, H, W = logits.shape
    assert acc.shape == logits.shape
    if nonlin == "softmax":
        check(lib().cf_tta_accumulate(_f32(logits), _f32(acc), B, K, H, W, int(flip_h), int(flip_w), float(weight), _stream()),
              "cf_tta_accumulate")
    else:
        check(lib().cf_tta_accumulate_nonlin(_f32(logits), _f32(acc), B, K, H, W, int(flip_h), int(flip_w), float(weight), _nonlin_code(nonlin),
                                             _stream()), "cf_tta_accumulate_nonlin")
    return acc


def tta_accumulate_window(logits, windows, acc, flip_h, flip_w, weight):
    """logits [B,K,c,c] of one flip variant, windows: device int32 [B,4] (crop_windows), acc [B,K,H,W]: acc[b][:, window b] += weight *
    flip(softmax(logits[b])); nothing outside the windows is touched (bits of tta_accumulate into a crop-sized buffer + pad2d inside)."""
    B, K, c, c2 = logits.shape
    if not isinstance(windows, torch.Tensor) or not windows.is_cuda or windows.dtype != torch.int32 or not windows.is_contiguous() \
            or tuple(windows.shape) != (B, 4):
        raise TypeError("windows must be a contiguous CUDA int32 tensor [B,4]")
    assert c == c2 and acc.dim() == 4 and acc.shape[:2] == (B, K), (logits.shape, acc.shape)
    H, W = acc.shape[2:]
    check(lib().cf_tta_accumulate_window(_f32(logits), windows.data_ptr(), _f32(acc), B, K, c, H, W, int(flip_h), int(flip_w), float(weight),
                                         _stream()), "cf_tta_accumulate_window")
    return acc


def flip2d(src, flip_h, flip_w):
    H, W = src.shape[-2:]
    N = src.numel() // (H * W)
    dst = torch.empty_like(src)
    check(lib().cf_flip2d(_f32(src), _f32(dst), N, H, W, int(flip_h), int(flip_w), _stream()), "cf_flip2d")
    return dst


def tile_accumulate(pred, gauss, agg, cnt, lx, ly):
    K, ph, pw = pred.shape
    _, X, Y = agg.shape
    check(lib().cf_tile_accumulate(_f32(pred), _opt(gauss), _f32(agg), _f32(cnt), K, X, Y, lx, ly, ph, pw, _stream()),
          "cf_tile_accumulate")


def tile_finalize(agg, cnt):
    K, X, Y = agg.shape
    probs = torch.empty_like(agg)
    seg = torch.empty((X, Y), dtype=torch.uint8, device=agg.device)
    check(lib().cf_tile_finalize(_f32(agg), _f32(cnt), _f32(probs), _u8(seg), K, X, Y, _stream()), "cf_tile_finalize")
    return seg, probs


def tile_gather(src, jobs, ph, pw):
    """src [N,C,X,Y]; jobs: device int32 [J,3] = (n, lx, ly) -> [J,C,ph,pw], dst[j] = src[n_j][:, lx_j:lx_j+ph, ly_j:ly_j+pw]."""
    N, C, X, Y = src.shape
    if not isinstance(jobs, torch.Tensor) or not jobs.is_cuda or jobs.dtype != torch.int32 or not jobs.is_contiguous() or jobs.dim() != 2 \
            or jobs.shape[1] != 3:
        raise TypeError("jobs must be a contiguous CUDA int32 tensor [J,3]")
    J = jobs.shape[0]
    dst = torch.empty((J, C, ph, pw), dtype=torch.float32, device=src.device)
    check(lib().cf_tile_gather(_f32(src), jobs.data_ptr(), _f32(dst), J, N, C, X, Y, ph, pw, _stream()), "cf_tile_gather")
    return dst


def tile_merge(pred, gauss, X, Y, lx, ly):
    """pred [N*len(lx)*len(ly),K,ph,pw] (slice-major, then tile order lx outer / ly inner), gauss [ph,pw] or None, lx / ly: the host step
    lists -> (seg uint8 [N,X,Y], probs [N,K,X,Y]); bit-identical to tile_accumulate per tile + tile_finalize per slice."""
    import ctypes
    J, K, ph, pw = pred.shape
    nx, ny = len(lx), len(ly)
    assert J % (nx * ny) == 0, (J, nx, ny)
    N = J // (nx * ny)
    probs = torch.empty((N, K, X, Y), dtype=torch.float32, device=pred.device)
    seg = torch.empty((N, X, Y), dtype=torch.uint8, device=pred.device)
    clx, cly = (ctypes.c_int * nx)(*[int(v) for v in lx]), (ctypes.c_int * ny)(*[int(v) for v in ly])
    check(lib().cf_tile_merge(_f32(pred), _opt(gauss), _f32(probs), _u8(seg), N, K, X, Y, ph, pw, ctypes.cast(clx, ctypes.c_void_p), nx,
                              ctypes.cast(cly, ctypes.c_void_p), ny, _stream()), "cf_tile_merge")
    return seg, probs


def tta_accumulate_3d(logits, acc, flip_d, flip_h, flip_w, weight, nonlin="softmax"):
    B, K, D, H, W = logits.shape
    assert acc.shape == logits.shape
    if nonlin == "softmax":
        check(lib().cf_tta_accumulate_3d(_f32(logits), _f32(acc), B, K, D, H, W, int(flip_d), int(flip_h), int(flip_w), float(weight),
                                         _stream()), "cf_tta_accumulate_3d")
    else:
        check(lib().cf_tta_accumulate_3d_nonlin(_f32(logits), _f32(acc), B, K, D, H, W, int(flip_d), int(flip_h), int(flip_w), float(weight),
                                                _nonlin_code(nonlin), _stream()), "cf_tta_accumulate_3d_nonlin")
    return acc


def flip3d(src, flip_d, flip_h, flip_w):
    D, H, W = src.shape[-3:]
    N = src.numel() // (D * H * W)
    dst = torch.empty_like(src)
    check(lib().cf_flip3d(_f32(src), _f32(dst), N, D, H, W, int(flip_d), int(flip_h), int(flip_w), _stream()), "cf_flip3d")
    return dst


def tile_accumulate_3d(pred, gauss, agg, cnt, lx, ly, lz):
    K, px, py, pz = pred.shape
    _, X, Y, Z = agg.shape
    check(lib().cf_tile_accumulate_3d(_f32(pred), _opt(gauss), _f32(agg), _f32(cnt), K, X, Y, Z, lx, ly, lz, px, py, pz, _stream()),
          "cf_tile_accumulate_3d")


def argmax_channels(x):
    B, K = x.shape[0], x.shape[1]
    HW = x.numel() // (B * K)
    out = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device)
    check(lib().cf_argmax_channels(_f32(x), _u8(out), B, K, HW, _stream()), "cf_argmax_channels")
    return out


def check_regions_class_order(order, K, who="regions_class_order"):
    """the K label values of a region head as a list of ints in 0..255"""
    order = [int(c) for c in order]
    if len(order) != K or any(c < 0 or c > 255 for c in order):
        raise ValueError("%s must hold one label in 0..255 per region channel (%d), got %r" % (who, K, order))
    return order


def region_labels(probs, regions_class_order):
    """probs [B,K,...] fp32 (one sigmoid channel per region) -> uint8 [B,...]: 0, overwritten by regions_class_order[i] where probs[:, i] > 0.5,
    i = 0..K-1 in that order (neural_network.py:749-751; the rule ensemble_merge applies to a mean)."""
    import ctypes
    B, K = probs.shape[0], probs.shape[1]
    order = check_regions_class_order(regions_class_order, K)
    HW = probs.numel() // max(B * K, 1)
    out = torch.empty((B,) + tuple(probs.shape[2:]), dtype=torch.uint8, device=probs.device)
    corder = (ctypes.c_uint8 * K)(*order)
    check(lib().cf_region_labels(_f32(probs), _u8(out), B, K, HW, ctypes.cast(corder, ctypes.c_void_p), _stream()), "cf_region_labels")
    return out


def window_attention(qk, v, bias_table, heads, window, shift):
    """Swin windowed cross-attention core: qk [B,2C,H,W] (q | k of one input), v [B,C,H,W] (of the other), bias_table [(2w-1)^2, heads]
    -> [B,C,H,W] (nnunet/lib/swin_cross_attention.py:13-112 without the projections)."""
    B, C, H, W = v.shape
    assert qk.shape == (B, 2 * C, H, W) and bias_table.shape == ((2 * window - 1) ** 2, heads)
    out = torch.empty_like(v)
    check(lib().cf_window_attention(_f32(qk), _f32(v), _f32(bias_table), _f32(out), B, C, H, W, heads, window, shift, _stream()), "cf_window_attention")
    return out


def frame_boxes(x):
    """x [N,H,W] uint8 or float32 on the device -> int32 [N,4] = (x1, y1, x2, y2) of the non-zero pixels per frame, -1 for empty frames
    (torchvision.ops.masks_to_boxes as processor.py:140-160 uses it)."""
    assert x.is_cuda and x.dim() == 3 and x.is_contiguous() and x.dtype in (torch.uint8, torch.float32)
    N, H, W = x.shape
    boxes = torch.empty((N, 4), dtype=torch.int32, device=x.device)
    check(lib().cf_frame_boxes(x.data_ptr(), int(x.dtype == torch.float32), boxes.data_ptr(), N, H, W, _stream()), "cf_frame_boxes")
    return boxes


def crop_windows(labels, crop, image):
    """labels uint8 [N,H,W] on the device -> (windows int32 [N,4] = (x_low, x_high, y_low, y_high), jobs int32 [N,3] = (n, y_low, x_low)):
    Processor.get_mean_centroid of each map on its own + adjust_cropping_window, on the device; `jobs` is tile_gather's job table."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise TypeError("labels must be a contiguous CUDA uint8 tensor [N,H,W]")
    N, H, W = labels.shape
    windows = torch.empty((N, 4), dtype=torch.int32, device=labels.device)
    jobs = torch.empty((N, 3), dtype=torch.int32, device=labels.device)
    check(lib().cf_crop_windows(labels.data_ptr(), windows.data_ptr(), jobs.data_ptr(), N, H, W, int(crop), int(image), _stream()), "cf_crop_windows")
    return windows, jobs


def sample_points(field, pts):
    """SpatialTransformerContour (integration.py:5-34): field [B,C,H,W], pts [B,2,P] (channel 0 along W, channel 1 along H) -> [B,C,P]."""
    B, C, H, W = field.shape
    assert pts.shape[0] == B and pts.shape[1] == 2
    P_ = pts.shape[2]
    out = torch.empty((B, C, P_), dtype=torch.float32, device=field.device)
    check(lib().cf_sample_points_2d(_f32(field), _f32(pts), _f32(out), B, C, H, W, P_, _stream()), "cf_sample_points_2d")
    return out


# ------------------------------------------------------------------------------------------------ export post-processing
def resize3d(src, new_shape, linear=(1, 1, 1)):
    """src [N,X,Y,Z] float32 -> [N,*new_shape]; per axis linear (order 1) or nearest (order 0); skimage 'edge' semantics."""
    N, X, Y, Z = src.shape
    X2, Y2, Z2 = (int(v) for v in new_shape)
    dst = torch.empty((N, X2, Y2, Z2), dtype=torch.float32, device=src.device)
    check(lib().cf_resize3d(_f32(src), _f32(dst), N, X, Y, Z, X2, Y2, Z2, int(linear[0]), int(linear[1]), int(linear[2]), _stream()),
          "cf_resize3d")
    return dst


def resize_labels(src, new_shape, linear=(1, 1, 1)):
    """batchgenerators' resize_segmentation(order=1) of the label maps src [N,X,Y,Z] float32 -> [N,*new_shape]: the largest label whose
    resized fp64 indicator reaches 0.5, else 0; per axis linear or nearest, as resize3d."""
    N, X, Y, Z = src.shape
    X2, Y2, Z2 = (int(v) for v in new_shape)
    src = src.contiguous()
    dst = torch.empty((N, X2, Y2, Z2), dtype=torch.float32, device=src.device)
    check(lib().cf_resize_labels(_f32(src), _f32(dst), N, X, Y, Z, X2, Y2, Z2, int(linear[0]), int(linear[1]), int(linear[2]), _stream()),
          "cf_resize_labels")
    return dst


def prev_stage_onehot(seg, classes, out):
    """Previous-stage labels -> one-hot network-input planes (nnunet/inference/predict.py:82-85) in one kernel: batchgenerators'
    resize_segmentation(seg, out.shape[1:], order=1) then to_one_hot(., classes).  seg: uint8 [X,Y,Z]; out: float32
    [len(classes), X2, Y2, Z2], contiguous -- typically the view `net_input[num_modalities:]`, written in place.  Returns `out`."""
    import ctypes
    classes = [int(c) for c in classes]
    if seg.dim() != 3 or out.dim() != 4 or out.shape[0] != len(classes):
        raise ValueError("prev_stage_onehot: seg must be [X,Y,Z] and out [len(classes),X2,Y2,Z2], got %s and %s for %d classes"
                         % (tuple(seg.shape), tuple(out.shape), len(classes)))
    if not classes or any(c < 0 or c > 255 for c in classes):
        raise ValueError("prev_stage_onehot: classes must be 1..255 label values in 0..255, got %r" % (classes,))
    if seg.device != out.device:
        raise ValueError("prev_stage_onehot: seg and out live on different devices")
    cls = (ctypes.c_uint8 * len(classes))(*classes)
    X, Y, Z = seg.shape
    _, X2, Y2, Z2 = out.shape
    check(lib().cf_prev_stage_onehot(_u8(seg, "seg"), X, Y, Z, _f32(out, "out"), X2, Y2, Z2, ctypes.cast(cls, ctypes.c_void_p), len(classes),
                                     _stream()), "cf_prev_stage_onehot")
    return out


ENSEMBLE_MAX_MEMBERS = 16


def _check_members(who, members, lo, hi):
    """lo..hi contiguous CUDA tensors [K,Z,Y,X] of one shape, dtype (float16 / float32) and device, K in 1..255 -> the first"""
    if not lo <= len(members) <= hi:
        raise ValueError("%s: %d members (%d..%d are supported)" % (who, len(members), lo, hi))
    for i, m in enumerate(members):
        if not isinstance(m, torch.Tensor) or not m.is_cuda:
            raise TypeError("%s: member %d must be a CUDA/HIP tensor (cineflow has no CPU path)" % (who, i))
    first = members[0]
    if first.dtype not in (torch.float16, torch.float32) or first.dim() != 4:
        raise ValueError("%s: members must be [K,Z,Y,X] float16 or float32, member 0 is %s %s" % (who, tuple(first.shape), first.dtype))
    for i, m in enumerate(members):
        if m.dtype != first.dtype or m.shape != first.shape or m.device != first.device:
            raise ValueError("%s: member %d is %s %s on %s, member 0 is %s %s on %s"
                             % (who, i, tuple(m.shape), m.dtype, m.device, tuple(first.shape), first.dtype, first.device))
        if not m.is_contiguous():
            raise ValueError("%s: member %d must be contiguous" % (who, i))
    if not 1 <= first.shape[0] <= 255:
        raise ValueError("%s: %d classes (1..255 are supported)" % (who, first.shape[0]))
    return first


def _check_placement(who, size, bbox_lo, full_shape):
    """the crop of `size` at bbox_lo must lie inside full_shape; returns bbox_lo as ints"""
    bbox_lo = tuple(int(v) for v in bbox_lo)
    if len(full_shape) != 3 or len(bbox_lo) != 3 or any(lo < 0 or lo + n > f for lo, n, f in zip(bbox_lo, size, full_shape)):
        raise ValueError("%s: members of size %s at %s do not fit into %s" % (who, tuple(size), bbox_lo, tuple(full_shape)))
    return bbox_lo


def _ensemble_merge_into(members, seg, bbox_lo, mean, regions_class_order):
    """cf_ensemble_merge on checked arguments: members [K,Z,Y,X] float16 / float32 -> labels into `seg` (uint8 [Zf,Yf,Xf], contiguous, every
    voxel written) and, when `mean` is a tensor like a member, the mean into it."""
    import ctypes
    K, Z, Y, X = members[0].shape
    Zf, Yf, Xf = seg.shape
    ptrs = (ctypes.c_void_p * len(members))(*[m.data_ptr() for m in members])
    order = None
    if regions_class_order is not None:
        order = ctypes.cast((ctypes.c_uint8 * K)(*regions_class_order), ctypes.c_void_p)
    check(lib().cf_ensemble_merge(ctypes.cast(ptrs, ctypes.c_void_p), len(members), int(members[0].dtype == torch.float32), K, Z, Y, X,
                                  _u8(seg, "seg"), Zf, Yf, Xf, int(bbox_lo[0]), int(bbox_lo[1]), int(bbox_lo[2]),
                                  None if mean is None else mean.data_ptr(), order, _stream()), "cf_ensemble_merge")


def ensemble_merge(members, full_shape=None, bbox_lo=(0, 0, 0), want_mean=False, regions_class_order=None):
    """nnunet/inference/ensemble_predictions.py merge_files on the device, one kernel: members, a list of 1..16 softmax volumes [K,Z,Y,X]
    of one shape, all float16 or all float32 -> (seg uint8 [Zf,Yf,Xf], mean [K,Z,Y,X] in the members' dtype or None).  The mean is numpy's
    np.mean(np.vstack([m[None] for m in members]), 0) bit for bit; seg is its argmax(0) -- or, with a regions_class_order, 0 overwritten by
    regions_class_order[i] where mean[i] > 0.5, in that order -- placed at bbox_lo inside zeros of full_shape (default: the members' own)."""
    members = list(members)
    first = _check_members("ensemble_merge", members, 1, ENSEMBLE_MAX_MEMBERS)
    full_shape = tuple(int(v) for v in (first.shape[1:] if full_shape is None else full_shape))
    bbox_lo = _check_placement("ensemble_merge", first.shape[1:], bbox_lo, full_shape)
    if regions_class_order is not None:
        regions_class_order = check_regions_class_order(regions_class_order, first.shape[0], "ensemble_merge: regions_class_order")
    seg = torch.empty(full_shape, dtype=torch.uint8, device=first.device)
    mean = torch.empty_like(first) if want_mean else None
    _ensemble_merge_into(members, seg, bbox_lo, mean, regions_class_order)
    return seg, mean


ENSEMBLE_PAIRS_MAX_MEMBERS = 8
ENSEMBLE_PAIRS_MAX = 28
ENSEMBLE_PAIRS_HIST_K = 16


def ensemble_pairs(members, pairs, gt, bbox_lo=(0, 0, 0), regions_class_order=None, out=None):
    """Every listed two-member ensemble of `members` against one ground truth, one kernel (cf_ensemble_pairs): members, a list of 2..8
    softmax volumes [K,Z,Y,X] of one shape, all float16 or all float32; pairs, a list of 1..28 (i, j) with i != j; gt, uint8 [Zf,Yf,Xf]
    -> (seg uint8 [P,Zf,Yf,Xf], hist int64 [P, 16 * 16 + 1]).  seg[p] is ensemble_merge([members[i], members[j]], gt.shape, bbox_lo,
    regions_class_order=...)[0] byte for byte and hist[p] is cf_label_confusion(seg[p], gt) at K = 16 count for count (hist[p, t * 16 + r];
    the last bin counts the voxels with a label >= 16 in either volume).  Each member is read once.  out: (seg, hist) tensors to write into
    (every element of both is written)."""
    import ctypes
    members = list(members)
    first = _check_members("ensemble_pairs", members, 2, ENSEMBLE_PAIRS_MAX_MEMBERS)
    K, Z, Y, X = first.shape
    pairs = [(int(i), int(j)) for i, j in pairs]
    if not 1 <= len(pairs) <= ENSEMBLE_PAIRS_MAX:
        raise ValueError("ensemble_pairs: %d pairs (1..%d are supported)" % (len(pairs), ENSEMBLE_PAIRS_MAX))
    for i, j in pairs:
        if i == j or not (0 <= i < len(members) and 0 <= j < len(members)):
            raise ValueError("ensemble_pairs: pair (%d, %d) does not name two of the %d members" % (i, j, len(members)))
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or gt.dim() != 3 or gt.device != first.device or not gt.is_contiguous():
        raise ValueError("ensemble_pairs: gt must be a contiguous uint8 [Zf,Yf,Xf] tensor on the members' device")
    Zf, Yf, Xf = gt.shape
    bbox_lo = _check_placement("ensemble_pairs", (Z, Y, X), bbox_lo, (Zf, Yf, Xf))
    order = None
    if regions_class_order is not None:
        regions_class_order = check_regions_class_order(regions_class_order, K, "ensemble_pairs: regions_class_order")
        order = ctypes.cast((ctypes.c_uint8 * K)(*regions_class_order), ctypes.c_void_p)
    P = len(pairs)
    bins = ENSEMBLE_PAIRS_HIST_K * ENSEMBLE_PAIRS_HIST_K + 1
    if out is None:
        seg = torch.empty((P, Zf, Yf, Xf), dtype=torch.uint8, device=first.device)
        hist = torch.empty((P, bins), dtype=torch.int64, device=first.device)
    else:
        seg, hist = out
        for t, shape, dtype, what in ((seg, (P, Zf, Yf, Xf), torch.uint8, "seg"), (hist, (P, bins), torch.int64, "hist")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != first.device or not t.is_contiguous():
                raise ValueError("ensemble_pairs: out %s must be a contiguous %s %s tensor on the members' device" % (what, shape, dtype))
    ptrs = (ctypes.c_void_p * len(members))(*[m.data_ptr() for m in members])
    flat = (ctypes.c_int * (2 * P))(*[v for ij in pairs for v in ij])
    check(lib().cf_ensemble_pairs(ctypes.cast(ptrs, ctypes.c_void_p), len(members), int(first.dtype == torch.float32), K, Z, Y, X,
                                  ctypes.cast(flat, ctypes.c_void_p), P, _u8(gt, "gt"), _u8(seg, "seg"), Zf, Yf, Xf, bbox_lo[0], bbox_lo[1],
                                  bbox_lo[2], order, hist.data_ptr(), _stream()), "cf_ensemble_pairs")
    return seg, hist


RESAMPLE_HIST_K = 16


def resample_argmax(src, new_shape, linear, full_shape=None, bbox_lo=(0, 0, 0), regions_class_order=None, want_probs=False, gt=None):
    """The export of one validated case in one kernel (cf_resample_argmax): src, a contiguous float32 CUDA tensor [K,X,Y,Z] (K in 1..255),
    resampled to new_shape as resize3d(src, new_shape, linear) resamples it, bit for bit (equal sizes copy) -> (seg, probs, hist).
    seg: uint8 [*full_shape] (default: new_shape), the arg-max over the channels (first maximum) -- or, with a regions_class_order, 0
    overwritten by regions_class_order[i] where channel i > 0.5, in that order -- placed at bbox_lo inside zeros.  probs (want_probs, else
    None): float16 [K,*new_shape], export.probabilities_as_stored of the resampled channels.  hist (gt given, else None): int64
    [16 * 16 + 1], cf_label_confusion(seg, gt) at K = 16 (hist[t * 16 + r]; the last bin counts the voxels with a label >= 16 in either
    volume); gt: contiguous uint8 [*full_shape] on src's device."""
    who = "resample_argmax"
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise TypeError("%s: src must be a CUDA/HIP tensor (cineflow has no CPU path)" % who)
    if src.dtype != torch.float32 or src.dim() != 4:
        raise ValueError("%s: src must be [K,X,Y,Z] float32, got %s %s" % (who, tuple(src.shape), src.dtype))
    if not src.is_contiguous():
        raise ValueError("%s: src must be contiguous" % who)
    K, X, Y, Z = src.shape
    if not 1 <= K <= 255:
        raise ValueError("%s: %d classes (1..255 are supported)" % (who, K))
    new_shape = tuple(int(v) for v in new_shape)
    if len(new_shape) != 3 or len(linear) != 3 or min(new_shape) < 1 or min(X, Y, Z) < 1:
        raise ValueError("%s: cannot resample %s to %s with linear = %r" % (who, (X, Y, Z), new_shape, tuple(linear)))
    full_shape = tuple(int(v) for v in (new_shape if full_shape is None else full_shape))
    bbox_lo = _check_placement(who, new_shape, bbox_lo, full_shape)
    order = None
    if regions_class_order is not None:
        regions_class_order = check_regions_class_order(regions_class_order, K, who + ": regions_class_order")
        order = ctypes.cast((ctypes.c_uint8 * K)(*regions_class_order), ctypes.c_void_p)
    hist = None
    if gt is not None:
        if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or tuple(gt.shape) != full_shape or gt.device != src.device \
                or not gt.is_contiguous():
            raise ValueError("%s: gt must be a contiguous uint8 %s tensor on src's device" % (who, full_shape))
        hist = torch.empty(RESAMPLE_HIST_K * RESAMPLE_HIST_K + 1, dtype=torch.int64, device=src.device)
    seg = torch.empty(full_shape, dtype=torch.uint8, device=src.device)
    probs = torch.empty((K,) + new_shape, dtype=torch.float16, device=src.device) if want_probs else None
    check(lib().cf_resample_argmax(src.data_ptr(), K, X, Y, Z, new_shape[0], new_shape[1], new_shape[2], int(bool(linear[0])),
                                   int(bool(linear[1])), int(bool(linear[2])), seg.data_ptr(), full_shape[0], full_shape[1], full_shape[2],
                                   bbox_lo[0], bbox_lo[1], bbox_lo[2], order, None if probs is None else probs.data_ptr(),
                                   None if gt is None else gt.data_ptr(), None if hist is None else hist.data_ptr(), _stream()),
          "cf_resample_argmax")
    return seg, probs, hist


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, order_z=0):
    """nnunet/preprocessing/preprocessing.py:111-200 on the device for the orders the export uses (0 and 1).  data: numpy or
    device tensor (c, x, y, z); returns the same kind.  Segmentations of order 0 are nearest-neighbour in every axis; data is
    linear in-plane and `order_z` along the anisotropic axis when do_separate_z."""
    was_numpy = not torch.is_tensor(data)
    t = torch.from_numpy(np.ascontiguousarray(data)) if was_numpy else data
    dtype_in = t.dtype
    assert t.dim() == 4 and len(new_shape) == 3, "data must be (c, x, y, z)"
    if tuple(t.shape[1:]) == tuple(int(v) for v in new_shape):
        return data
    if order not in (0, 1) or order_z not in (0, 1):
        raise NotImplementedError("export resampling is built for interpolation orders 0 and 1 (got %s / %s)" % (order, order_z))
    if is_seg and order != 0:
        raise NotImplementedError("segmentation resampling is built for order 0")
    dev = torch.device("cuda", torch.cuda.current_device())
    lin = [int(order)] * 3
    if do_separate_z:
        assert len(axis) == 1, "only one anisotropic axis supported"
        lin[int(axis[0])] = int(order_z)
    out = resize3d(t.to(dev, dtype=torch.float32).contiguous(), new_shape, lin)
    if is_seg:
        out = out.round()
    out = out.to(dtype_in)
    return out.cpu().numpy() if was_numpy else out


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """nnunet/postprocessing/connected_components.py:51-107 on the device.  image: uint8 device tensor [Z,Y,X] or [Y,X]
    (modified in place); for_which_classes: ints or tuples of ints (joint regions) or None (all foreground labels).
    Returns (image, largest_removed, kept_size) like the reference."""
    import ctypes
    assert image.dtype == torch.uint8 and image.is_cuda and image.is_contiguous()
    shape = tuple(image.shape)
    D, H, W = (1,) * (3 - len(shape)) + shape
    n = image.numel()
    if for_which_classes is None:
        for_which_classes = [int(v) for v in torch.unique(image).tolist() if v > 0]
    assert 0 not in for_which_classes, "cannot remove background"
    labels = torch.empty(n, dtype=torch.int32, device=image.device)
    counts = torch.empty(n, dtype=torch.int32, device=image.device)
    changed = torch.zeros(1, dtype=torch.int32, device=image.device)
    largest_removed, kept_size = {}, {}
    for c in for_which_classes:
        key = tuple(c) if isinstance(c, (list, tuple)) else c
        vals = list(key) if isinstance(key, tuple) else [key]
        cls = (ctypes.c_uint8 * len(vals))(*[int(v) for v in vals])
        check(lib().cf_cc_init(_u8(image), labels.data_ptr(), n, ctypes.cast(cls, ctypes.c_void_p), len(vals), _stream()), "cf_cc_init")
        while True:
            changed.zero_()
            for _ in range(8):
                check(lib().cf_cc_sweep(labels.data_ptr(), D, H, W, changed.data_ptr(), _stream()), "cf_cc_sweep")
            if int(changed.item()) == 0:
                break
        counts.zero_()
        check(lib().cf_cc_count(labels.data_ptr(), counts.data_ptr(), n, _stream()), "cf_cc_count")
        sizes = counts[counts > 0]
        largest_removed[key] = None
        kept_size[key] = None
        if sizes.numel() > 0:
            max_count = int(sizes.max().item())
            kept_size[key] = max_count * volume_per_voxel
            thr = -1.0 if minimum_valid_object_size is None else float(minimum_valid_object_size[key])
            gone = sizes[sizes != max_count]
            if thr >= 0:
                gone = gone[gone.double() * volume_per_voxel < thr]
            if gone.numel() > 0:
                largest_removed[key] = int(gone.max().item()) * volume_per_voxel
            check(lib().cf_cc_remove(_u8(image), labels.data_ptr(), counts.data_ptr(), n, max_count, float(volume_per_voxel), thr, _stream()),
                  "cf_cc_remove")
    return image, largest_removed, kept_size


# ------------------------------------------------------------------------------------------------ determine_postprocessing (csrc/cc_label.hip)
PP_KMAX = 16


def _region_table(region_of):
    """dict {label value: region id} or a sequence of 256 region ids -> ctypes uint8 [256] (a host table; region 0 = outside)"""
    import ctypes
    tab = [0] * 256
    if isinstance(region_of, dict):
        for k, v in region_of.items():
            tab[int(k)] = int(v)
    else:
        tab = [int(v) for v in region_of]
        assert len(tab) == 256, "region_of must name all 256 label values"
    assert tab[0] == 0 and all(0 <= v < 256 for v in tab), "region ids are 0..255 and label 0 is outside"
    return (ctypes.c_uint8 * 256)(*tab)


def _dhw(t):
    shape = tuple(t.shape)
    assert 1 <= len(shape) <= 3, "2-D or 3-D label maps"
    return (1,) * (3 - len(shape)) + shape


def _host_array(ctype, values, K, fill):
    """values: None, or a dict / sequence indexed by class -> ctypes array [K]"""
    if values is None:
        return None
    vals = [fill] * K
    for k, v in (values.items() if isinstance(values, dict) else enumerate(values)):
        vals[int(k)] = v
    return (ctype * K)(*vals)


def connected_component_labels(image, region_of):
    """Every connected component (face neighbours, scipy.ndimage.label's default) of every region of a uint8 label map in one call:
    int32 tensor of image's shape, 0 outside, else 1 + the smallest flat voxel index of the component.  region_of: {label: region id};
    neighbours are connected iff their region ids are equal and non-zero."""
    import ctypes
    D, H, W = _dhw(image)
    labels = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    tab = _region_table(region_of)
    check(lib().cf_cc_label(_u8(image, "image"), labels.data_ptr(), D, H, W, ctypes.cast(tab, ctypes.c_void_p), _stream()), "cf_cc_label")
    return labels


def connected_component_sizes(labels, image, region_of, alive=None):
    """-> (counts int32 [n] indexed by label - 1, region_max int32 [256][, region_max_alive int32 [256] when `alive` is given])"""
    import ctypes
    n = image.numel()
    assert labels.dtype == torch.int32 and labels.is_cuda and labels.is_contiguous() and labels.numel() == n
    counts = torch.empty(n, dtype=torch.int32, device=image.device)
    mx = torch.empty(256 * (2 if alive is not None else 1), dtype=torch.int32, device=image.device)
    tab = _region_table(region_of)
    check(lib().cf_cc_sizes(labels.data_ptr(), _u8(image, "image"), ctypes.cast(tab, ctypes.c_void_p), None if alive is None else _u8(alive, "alive"),
                            n, counts.data_ptr(), mx.data_ptr(), None if alive is None else mx[256:].data_ptr(), _stream()), "cf_cc_sizes")
    return (counts, mx) if alive is None else (counts, mx[:256], mx[256:])


def pp_confusion(pred, gt, K, labels_fg, counts_fg, max_fg, labels_cls, counts_cls, max_cls, max_cls_alive, volume_per_voxel, min_valid=None,
                 z_skip=None):
    """{TP, FP, FN} of every class < K for the raw prediction and its three filtered variants -> int64 device tensor [4, K, 3].
    min_valid: None or {0: foreground threshold, c: class threshold} (missing entries: always remove); z_skip: None or {class: first slice}."""
    import ctypes
    D, H, W = _dhw(pred)
    assert tuple(pred.shape) == tuple(gt.shape), "Shape mismatch: {} and {}".format(pred.shape, gt.shape)
    out = torch.empty((4, K, 3), dtype=torch.int64, device=pred.device)
    mv = _host_array(ctypes.c_double, min_valid, K, -1.0)
    zs = _host_array(ctypes.c_int, z_skip, K, 0)
    check(lib().cf_pp_confusion(_u8(pred, "pred"), _u8(gt, "gt"), D, H, W, K, labels_fg.data_ptr(), counts_fg.data_ptr(), max_fg.data_ptr(),
                                labels_cls.data_ptr(), counts_cls.data_ptr(), max_cls.data_ptr(), max_cls_alive.data_ptr(), float(volume_per_voxel),
                                None if mv is None else ctypes.cast(mv, ctypes.c_void_p), None if zs is None else ctypes.cast(zs, ctypes.c_void_p),
                                out.data_ptr(), _stream()), "cf_pp_confusion")
    return out


def cc_apply(src, K, do_fg, classes, labels_fg, counts_fg, max_fg, labels_cls, counts_cls, max_cls, volume_per_voxel, min_valid=None, out=None):
    """The filtered image for "foreground step yes/no + the single classes in `classes`" from the label maps of one case."""
    import ctypes
    out = torch.empty_like(src) if out is None else out
    bits = 0
    for c in classes:
        assert 1 <= int(c) < K, "class %r outside 1..%d" % (c, K - 1)
        bits |= 1 << int(c)
    mv = _host_array(ctypes.c_double, min_valid, K, -1.0)
    ptr = lambda t: None if t is None else t.data_ptr()                                  # noqa: E731
    check(lib().cf_cc_apply(_u8(src, "src"), _u8(out, "out"), src.numel(), K, int(bool(do_fg)), bits, ptr(labels_fg), ptr(counts_fg), ptr(max_fg),
                            ptr(labels_cls), ptr(counts_cls), ptr(max_cls), float(volume_per_voxel), None if mv is None else ctypes.cast(mv, ctypes.c_void_p),
                            _stream()), "cf_cc_apply")
    return out


# ------------------------------------------------------------------------------------------------ voxels by rank (csrc/dataset.hip)
class RankIndex(object):
    """The block prefixes of one count pass over `key` (cf_select_count): what select_coords / select_values search.  values None: the one
    row of the predicate `key > 0`; else one row per listed value, `key == value`.  totals: numpy int64, one per row (the only read-back)."""

    def __init__(self, key, values=None):
        import ctypes
        ptr = _f32(key, "key")
        self.key, self.n = key, key.numel()
        self.values = None if values is None else [float(v) for v in values]
        rows = 1 if values is None else len(self.values)
        nb = max(lib().cf_select_blocks(self.n), 1)
        self.prefix = torch.empty((max(rows, 1), nb), dtype=torch.int32, device=key.device)
        totals = torch.empty(max(rows, 1), dtype=torch.int64, device=key.device)
        vals = None if values is None else ctypes.cast((ctypes.c_float * max(rows, 1))(*self.values), ctypes.c_void_p)
        check(lib().cf_select_count(ptr, self.n, vals, rows, int(values is None), self.prefix.data_ptr(), totals.data_ptr(), _stream()), "cf_select_count")
        self.totals = totals.cpu().numpy()

    def row(self, value):
        if self.values is None:
            assert value is None, "this index holds the `> 0` predicate"
            return 0
        return self.values.index(float(value))


def label_counts(seg, values):
    """np.array([(seg == v).sum() for v in values]) of a float32 device volume (at most 16 values) -> numpy int64."""
    return RankIndex(seg, values).totals


def _select(key, value, ranks, src, index):
    index = RankIndex(key, None if value is None else [value]) if index is None else index
    assert index.key.data_ptr() == key.data_ptr() and index.n == key.numel(), "the index was counted over another volume"
    row = index.row(value)
    total = int(index.totals[row])
    if not torch.is_tensor(ranks):
        ranks = torch.from_numpy(np.ascontiguousarray(np.asarray(ranks, dtype=np.int64)).reshape(-1))
    K = ranks.numel()
    if K and not ranks.is_cuda and (int(ranks.min()) < 0 or int(ranks.max()) >= total):
        raise IndexError("rank out of bounds: %d voxels match" % total)
    ranks = ranks.to(key.device, dtype=torch.int64).contiguous()
    if src is not None:
        assert src.numel() == key.numel(), "src and key must have the same number of voxels"
        out = torch.empty(K, dtype=torch.float32, device=key.device)
        args = (_f32(src, "src"), out.data_ptr(), None, 0, 0, 0)
    else:
        assert key.dim() == 3, "select_coords takes a 3-D volume"
        out = torch.empty((K, 3), dtype=torch.int64, device=key.device)
        args = (None, None, out.data_ptr()) + tuple(key.shape)
    if K == 0:              # (an empty tensor has no address to hand over; the call would launch nothing)
        return out
    check(lib().cf_select_rank(_f32(key, "key"), key.numel(), int(value is None), 0.0 if value is None else float(value), index.prefix[row].data_ptr(),
                               ranks.data_ptr() if K else None, K, *args, _stream()), "cf_select_rank")
    return out


def select_coords(seg, value, ranks, index=None):
    """np.argwhere(seg == value)[ranks] of a float32 device volume [X, Y, Z] -> int64 device tensor [K, 3].  ranks: numpy or tensor, any
    order, duplicates allowed.  index: a RankIndex over `seg` that lists `value` (saves the count pass when several classes are asked)."""
    return _select(seg, value, ranks, None, index)


def select_values(src, key, ranks, index=None):
    """src[key > 0][ranks] of two float32 device arrays of the same size -> float32 device tensor [K]."""
    return _select(key, None, ranks, src, index)


# ---------------------------------------------------------------- DEFLATE and CRC-32 of a device buffer (csrc/deflate.hip)
def deflate_chunk_bytes():
    """Bytes of input that cf_deflate compresses on their own (one workgroup, one run of non-final blocks)."""
    return int(lib().cf_deflate_chunk_bytes())


def deflate_bound(n):
    """Bytes that the stream of n input bytes never exceeds: n + 5 ceil(n / chunk)."""
    size = int(lib().cf_deflate_bound(int(n)))
    if size < 0:
        check(size, "cf_deflate_bound")
    return size


def _as_bytes(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError("%s must be a device tensor" % name)
    return t.contiguous().reshape(-1).view(torch.uint8)


def deflate(t, out=None, ws=None, out_bytes=None):
    """RFC 1951 blocks of a device tensor's bytes (C order), without the final block: -> (out uint8 [deflate_bound(n)], out_bytes int64 [1]),
    both on the device; the stream is out[:out_bytes].  Nothing is read back and nothing synchronises.  out / ws / out_bytes: the
    caller's buffers (tests pass guarded ones); by default they are allocated here."""
    b = _as_bytes(t, "deflate: t")
    n = b.numel()
    h = lib()
    out = torch.empty(max(deflate_bound(n), 1), dtype=torch.uint8, device=b.device) if out is None else out
    out_bytes = torch.empty(1, dtype=torch.int64, device=b.device) if out_bytes is None else out_bytes
    ws = torch.empty(int(h.cf_deflate_workspace_bytes(n)), dtype=torch.uint8, device=b.device) if ws is None else ws
    if n == 0:              # (an empty tensor has no address to hand over)
        out_bytes.zero_()
        return out, out_bytes
    check(h.cf_deflate(b.data_ptr(), n, out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), out_bytes.data_ptr(), _stream()), "cf_deflate")
    return out, out_bytes


def crc32(t, ws=None, crc=None):
    """zlib.crc32 of a device tensor's bytes -> int64 device tensor [1] (the low 32 bits; nothing is read back)."""
    b = _as_bytes(t, "crc32: t")
    n = b.numel()
    h = lib()
    crc = torch.zeros(1, dtype=torch.int64, device=b.device) if crc is None else crc
    if n == 0:
        crc.zero_()
        return crc
    ws = torch.empty(int(h.cf_crc32_workspace_bytes(n)), dtype=torch.uint8, device=b.device) if ws is None else ws
    check(h.cf_crc32(b.data_ptr(), n, ws.data_ptr(), ws.numel(), crc.data_ptr(), _stream()), "cf_crc32")
    return crc
