"""Who picks the kernel: one object owns a convolution's device-side weight forms and chooses the kernel of every call.

`PackedConv` (Conv2d, _Linear, the attention projections, the depth taps of the composed Conv3d, the fused SepConvGRU gates),
`PackedConvT` (the k2s2 transposed convolution, per depth tap for ConvTranspose3d) and `PackedConv3d` (Conv3d's two native kernels) are the
only places outside ops.py that read ops.CONV_MODE and ops.f16s_dynamic_ok (the probes of the deferred-norm decisions test the mode inside
ops.py).  The layer classes of nn.py / models.py / mtl.py hold one of these per weight and never touch another layer's packed tensors.
Route of a PackedConv call, first match:
    0. direct fp32 (conv_direct.hip)   built with direct=True (Conv2d alone), set_conv_mode("f16s"), a plain call (no x2 / act / out / alpha /
                                      bias override): ops.small_cout_supported shapes without statistics, ops.small_cin_supported ones without res
    1. row Winograd (conv_wino.hip)   built with wino=True, 3x3 / stride 1 / pad 1, Cout in whole 128-channel blocks (or a last block >= 96),
                                      16-byte aligned inputs, ops.wino_ok for the call's shape
    2. f16 hi/lo split (conv_f16s.hip) ops.f16s_supported kernel shape, set_conv_mode("f16s"), ops.f16s_dynamic_ok for the inputs AND the
                                      destination (all channels of `out`): an oversized destination sample takes 3 instead of raising in the library
    3. exact fp32 MFMA (conv.hip)      everything else
Route of a PackedConv3d call: cf_conv3d_f16s for (1|3, 3, 3) kernels, cf_conv3d_pw_f16s for a (1, 1, 1) kernel without x2, each under
set_conv_mode("f16s") and its ops.*_ok probe; None otherwise (Conv3d then runs its composition of 2-D convolutions).
"""
from . import ops

OWN = object()          # `bias=OWN`: the layer's own bias (None is a valid override: no bias)


def split_key(x, x2, chunk):
    """key of the split-aware packing a cat[x, x2] call needs: x's channel count when it is no whole number of chunks, else None"""
    c1 = x.shape[1]
    return c1 if (x2 is not None and c1 % chunk) else None


class PackedConv:
    """weight [Cout,Cin,KH,KW] in every form a kernel reads: the fp32 transposed matrix, the f16-split packing per split key (the plain one
    at construction, split ones on first use) and, for wino=True layers of an eligible shape, the Winograd packing per split key (on first use).
    direct=True: a plain call tries the two direct fp32 kernels (HBM-bound layers: the stems, the flow heads) on the checkpoint layout first"""

    def __init__(self, weight, bias=None, stride=1, pad=(0, 0), wino=False, direct=False):
        self.weight, self.bias, self.stride, self.pad, self.direct = weight, bias, stride, tuple(pad), direct
        self.cout, self.cin, self.kh, self.kw = weight.shape
        self.wt = ops.prep_conv_weight(weight)
        self.f16s = ops.f16s_supported(self.kh, self.kw, stride, self.pad)
        self.chunk = ops.f16s_chunk(self.kh, self.kw)
        self._pk, self._wino_pk = {}, {}
        if self.f16s:
            self.packed(None)
        # 3x3 / stride 1 layers with whole 128-channel output blocks (or a last block >= 96) may take the row-Winograd kernel
        # (ops.wino_ok decides per call shape)
        self.wino = bool(wino and self.f16s and (self.kh, self.kw) == (3, 3) and stride == 1
                         and (self.cout % 128 == 0 or (self.cout > 128 and self.cout % 128 >= 96)))

    def packed(self, key):
        """(packed fp16 tensor, scale exponent) of pack_conv_weight_f16s for a split key"""
        if key not in self._pk:
            self._pk[key] = ops.pack_conv_weight_f16s(self.weight, c1=key)
        return self._pk[key]

    def packed_wino(self, key):
        if key not in self._wino_pk:
            self._wino_pk[key] = ops.pack_conv_weight_wino(self.weight, c1=key)
        return self._wino_pk[key]

    @property
    def scale(self):
        """scale exponent s of the f16-split packing (the packed values are 2^s * w)"""
        return self.packed(None)[1]

    def __call__(self, x, x2=None, act=None, res=None, out=None, out_coff=0, alpha=1.0, bias=OWN, stats_groups=None):
        """act(alpha * conv(cat[x, x2]) + bias) + res into channels [out_coff, out_coff + Cout) of `out`.  stats_groups=G: returns (out, ws)
        with the GroupNorm statistics of `out` when an f16 kernel fused them, else (out, None)."""
        kh, kw, cout = self.kh, self.kw, self.cout
        if self.direct and ops.CONV_MODE == "f16s" and x2 is None and act is None and out is None and alpha == 1.0 and bias is OWN:
            if not stats_groups and ops.small_cout_supported(cout, kh, kw, self.stride, self.pad):
                return ops.conv2d_small_cout(x, self.weight, self.bias, res)                          # the flow heads
            if res is None and ops.small_cin_supported(self.cin, kh, kw, self.stride, self.pad, stats_groups):
                return ops.conv2d_small_cin(x, self.weight, self.bias, stats_groups)                  # the stems
        if bias is OWN:
            bias = self.bias
        if self.f16s and ops.CONV_MODE == "f16s":
            ohw = ((x.shape[2] + 2 * self.pad[0] - kh) // self.stride + 1) * ((x.shape[3] + 2 * self.pad[1] - kw) // self.stride + 1)
            if ops.f16s_dynamic_ok(x, x2, kh, out_sample_elems=(cout if out is None else out.shape[1]) * ohw, out_hw=ohw):
                key = split_key(x, x2, self.chunk)
                if (self.wino and x.data_ptr() % 16 == 0 and (x2 is None or x2.data_ptr() % 16 == 0)
                        and ops.wino_ok(x.shape[0], x.shape[1], 0 if x2 is None else x2.shape[1], x.shape[2], x.shape[3], cout)):
                    wpk, s = self.packed_wino(key)
                    return ops.conv2d_wino(x, wpk, s, bias, cout, x2=x2, act=act, res=res, out=out, out_coff=out_coff, alpha=alpha,
                                           stats_groups=stats_groups)
                wpk, s = self.packed(key)
                return ops.conv2d_f16s(x, wpk, s, bias, cout, kh, kw, self.stride, self.pad, x2=x2, act=act, res=res, out=out,
                                       out_coff=out_coff, alpha=alpha, stats_groups=stats_groups)
        y = ops.conv2d(x, self.wt, bias, cout, kh, kw, self.stride, self.pad, x2=x2, act=act, res=res, out=out, out_coff=out_coff, alpha=alpha)
        return (y, None) if stats_groups else y

    def prenorm_ok(self, x):
        """can this convolution take the RAW convolution output x with its normalisation + activation deferred (applied while the tile is
        staged)?  3x3 / stride 1 only; on the Winograd kernel where that takes the shape, else on conv_f16s' vector-staging shapes"""
        if not ((self.kh, self.kw) == (3, 3) and self.stride == 1 and self.f16s and x.data_ptr() % 16 == 0):
            return False
        B, C, H, W = x.shape
        return (self.wino and ops.wino_ok(B, C, 0, H, W, self.cout, prenorm=True)) or ops.prenorm_ok(x, self.cout)

    def prenorm(self, x, coef, slope, stats_groups=None):
        """conv(act((x - mean) * scale + shift)) with coef from ops.group_norm_coef; slope < 0: GELU.  Caller checked prenorm_ok(x)."""
        B, C, H, W = x.shape
        if self.wino and ops.wino_ok(B, C, 0, H, W, self.cout, prenorm=True):
            wpk, s = self.packed_wino(None)
            return ops.conv2d_wino_prenorm(x, coef, slope, wpk, s, self.bias, self.cout, stats_groups=stats_groups)
        wpk, s = self.packed(None)
        return ops.conv2d_f16s_prenorm(x, coef, slope, wpk, s, self.bias, self.cout, stats_groups=stats_groups)


class PackedConvT:
    """weight [Cin,Cout,2,2] of a kernel 2 / stride 2 transposed convolution: the f16-split packing of its GEMM (rows m = co*4 + dy*2 + dx)
    for the scatter kernel, the checkpoint layout for the fp32 kernel"""

    def __init__(self, weight, bias=None):
        self.weight, self.bias = weight, bias
        self.cin, self.cout = weight.shape[0], weight.shape[1]
        self.wpk, self.scale = ops.pack_conv_weight_f16s(weight.permute(1, 2, 3, 0).reshape(self.cout * 4, self.cin, 1, 1))

    def __call__(self, x, out=None, out_coff=0, stats_groups=None):
        """returns as PackedConv.__call__; the destination sample of the scatter is 4x the input map"""
        hw = x.shape[2] * x.shape[3]
        if ops.CONV_MODE == "f16s" and ops.f16s_dynamic_ok(x, None, 1, out_sample_elems=(self.cout if out is None else out.shape[1]) * 4 * hw, out_hw=hw):
            return ops.conv_transpose2d_k2s2_f16s(x, self.wpk, self.scale, self.bias, self.cout, out=out, out_coff=out_coff, stats_groups=stats_groups)
        y = ops.conv_transpose2d_k2s2(x, self.weight, self.bias, out=out, out_coff=out_coff)
        return (y, None) if stats_groups else y


class PackedConv3d:
    """weight [Cout,Cin,KD,KH,KW] of a Conv3d on the native 3-D kernels: the f16-split packing of conv3d_f16s.hip per split key and the one of
    conv3d_pw_f16s.hip, each on first use"""

    def __init__(self, weight, bias, stride):
        self.weight, self.bias, self.stride = weight, bias, tuple(stride)
        self.cout, self.ks = weight.shape[0], tuple(weight.shape[2:])
        self._pk, self._pw = {}, None

    def __call__(self, x, x2=None, stats_groups=None):
        """conv(cat[x, x2]) + bias on NCDHW tensors: (out, ws) with stats_groups, else out -- or None: neither kernel takes the call
        (set_conv_mode("f32"), one-term mode, declined shapes)"""
        if ops.CONV_MODE != "f16s":
            return None
        B, C, D, H, W = x.shape
        if self.ks[1:] == (3, 3) and ops.conv3d_f16s_ok(B, C, 0 if x2 is None else x2.shape[1], D, H, W, self.cout, self.ks, self.stride):
            key = split_key(x, x2, 16)
            if key not in self._pk:
                self._pk[key] = ops.pack_conv3d_weight_f16s(self.weight, c1=key)
            wpk, s = self._pk[key]
            return ops.conv3d_f16s(x, wpk, s, self.bias, self.cout, self.ks, self.stride, x2=x2, stats_groups=stats_groups)
        if self.ks == (1, 1, 1) and x2 is None and ops.conv3d_pw_f16s_ok(B, C, D, H, W, self.cout, self.stride):
            if self._pw is None:
                self._pw = ops.pack_conv3d_pw_weight_f16s(self.weight)
            wpk, s = self._pw
            return ops.conv3d_pw_f16s(x, wpk, s, self.bias, self.cout, self.stride, stats_groups=stats_groups)
        return None
