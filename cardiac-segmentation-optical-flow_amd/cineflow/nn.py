"""Host-side mirror of the reference's layer library, executing on the HIP C ABI.

Each class keeps the reference class name, constructor arguments and ``state_dict`` key names (SURVEY.md
appendix A), so a reference checkpoint (or the seeded fill of cineflow.weights) loads unchanged; `forward`
issues hand-written HIP kernels only (cineflow.ops).  Tensors are NCHW float32 on the GPU; tokens stay
channel-first ([B,C,N]) so the reference's permute/contiguous round trips never happen and nn.Linear becomes a
1x1 convolution on the same implicit-GEMM kernel.  `file:line` citations are relative to /root/reference.
"""
import math
from typing import NamedTuple

import torch

from . import ops
from .convroute import OWN, PackedConv, PackedConv3d, PackedConvT


class Module:
    """Minimal module tree: parameters are declared with `_param(name, shape)`, children are attributes that
    are Modules, lists of Modules, or dicts {index: Module} (for nn.Sequential slots)."""

    def __init__(self):
        object.__setattr__(self, "_shapes", {})
        object.__setattr__(self, "_p", {})

    def _param(self, name, shape):
        self._shapes[name] = tuple(int(s) for s in shape)

    def _children(self):
        for k, v in self.__dict__.items():
            if k.startswith("_"):
                continue
            if isinstance(v, Module):
                yield k, v
            elif isinstance(v, (list, tuple)):
                for i, m in enumerate(v):
                    if isinstance(m, Module):
                        yield "%s.%d" % (k, i), m
            elif isinstance(v, dict):
                for i, m in v.items():
                    if isinstance(m, Module):
                        yield "%s.%s" % (k, i), m

    def state_shapes(self, prefix=""):
        out = {prefix + k: v for k, v in self._shapes.items()}
        for name, child in self._children():
            out.update(child.state_shapes(prefix + name + "."))
        return out

    def load_state_dict(self, sd, device, prefix="", strict=True):
        """sd: mapping name -> CPU/GPU tensor with the reference's key names."""
        mine = {}
        for k, shape in self._shapes.items():
            full = prefix + k
            if full not in sd:
                if strict:
                    raise KeyError("missing parameter %s" % full)
                continue
            t = sd[full]
            if tuple(t.shape) != shape:
                raise ValueError("shape mismatch for %s: %s vs %s" % (full, tuple(t.shape), shape))
            mine[k] = t.detach().to(device=device, dtype=torch.float32).contiguous()
        self._p.update(mine)
        self._prepare()
        for name, child in self._children():
            child.load_state_dict(sd, device, prefix + name + ".", strict)
        return self

    def _prepare(self):
        """Hook: derive device-side layouts (packed weights) after loading."""

    @classmethod
    def from_tensors(cls, weight, bias, *args, **kwargs):
        """a weight / bias layer (constructor arguments as given) holding these device tensors instead of a checkpoint's: the derived
        layers (a folded BatchNorm, a 1x1 view of another layer's weights)"""
        m = cls(*args, bias=bias is not None, **kwargs)
        m._p["weight"] = weight.contiguous()
        if bias is not None:
            m._p["bias"] = bias.contiguous()
        m._prepare()
        return m

    def __call__(self, *a, **k):
        return self.forward(*a, **k)


# --------------------------------------------------------------------------------------------- basic layers
class Conv2d(Module):
    """nn.Conv2d.  The device forms of the weight and the choice of kernel belong to its convroute.PackedConv (`_packed`)."""

    def __init__(self, cin, cout, kernel_size=3, stride=1, padding=0, bias=True):
        super().__init__()
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        pd = (padding, padding) if isinstance(padding, int) else tuple(padding)
        # per-axis strides (the plans' anisotropic pooling stages, e.g. (2, 1) at the bottom of the ACDC 2-D U-Net): the kernels take one
        # stride for both axes, so an unequal pair runs at stride 1 and the output is subsampled -- those stages are a few pixels wide
        self.sub = None
        if not isinstance(stride, int):
            sy, sx = (int(v) for v in stride)
            if sy == sx:
                stride = sy
            else:
                assert ks[0] % 2 == 1 and ks[1] % 2 == 1 and pd == (ks[0] // 2, ks[1] // 2), "per-axis strides are built for 'same' padded kernels"
                self.sub, stride = (sy, sx), 1
        self.cin, self.cout, self.ks, self.stride, self.pad = cin, cout, ks, stride, pd
        self._param("weight", (cout, cin, ks[0], ks[1]))
        if bias:
            self._param("bias", (cout,))

    def _prepare(self):
        if "weight" in self._p:
            self._packed = PackedConv(self._p["weight"], self._p.get("bias"), self.stride, self.pad, wino=self.sub is None, direct=True)

    @property
    def _ws(self):
        """scale exponent s of the layer's f16-split packing (packed values are 2^s * w)"""
        return self._packed.scale

    def prenorm_ok(self, x):
        """PackedConv.prenorm_ok; never for a subsampled (per-axis stride) layer"""
        return self.sub is None and self._packed.prenorm_ok(x)

    def prenorm(self, x, coef, slope, stats_groups=None):
        return self._packed.prenorm(x, coef, slope, stats_groups)

    def forward(self, x, x2=None, act=None, res=None, out=None, out_coff=0, stats_groups=None, alpha=1.0, bias=OWN):
        """stats_groups=G: returns (out, ws) with the GroupNorm statistics of `out` when the f16 kernel can fuse them, else (out, None)."""
        if self.sub is not None:
            assert act is None and res is None and out is None, "per-axis strides: plain convolution only"
            y = self._packed(x, x2, alpha=alpha, bias=bias)
            y = y[:, :, ::self.sub[0], ::self.sub[1]].contiguous()
            return (y, None) if stats_groups else y
        return self._packed(x, x2, act, res, out, out_coff, alpha, bias, stats_groups)


class ConvTranspose2d(Module):
    """nn.ConvTranspose2d(kernel_size = stride = (2, 2)) on its convroute.PackedConvT; (2, 1) / (1, 2) for the plans' anisotropic stages
    (generic_UNet.py:343-344): a 1x1 convolution to Cout * k rows of the GEMM whose outputs are interleaved along the up-sampled axis by a
    strided copy (bottom-of-the-net maps of a few pixels)."""

    def __init__(self, cin, cout, bias=True, kernel_size=(2, 2)):
        super().__init__()
        self.cin, self.cout, self.ks = cin, cout, tuple(int(v) for v in kernel_size)
        assert self.ks in ((2, 2), (2, 1), (1, 2)), "transposed kernel (2,2), (2,1) or (1,2)"
        self._param("weight", (cin, cout) + self.ks)
        if bias:
            self._param("bias", (cout,))

    def _prepare(self):
        if "weight" in self._p:
            w, b = self._p["weight"], self._p.get("bias")  # [Cin,Cout,kh,kw] -> GEMM rows m = co*kh*kw + dy*kw + dx
            if self.ks == (2, 2):
                self._packed = PackedConvT(w, b)
            else:
                k = self.ks[0] * self.ks[1]
                self._w1 = Conv2d.from_tensors(w.permute(1, 2, 3, 0).reshape(self.cout * k, self.cin, 1, 1),
                                               None if b is None else b.repeat_interleave(k), self.cin, self.cout * k, 1)

    def _forward_aniso(self, x):
        B, _, H, W = x.shape
        y = self._w1(x).view(B, self.cout, self.ks[0], self.ks[1], H, W)
        return y.permute(0, 1, 4, 2, 5, 3).reshape(B, self.cout, H * self.ks[0], W * self.ks[1]).contiguous()

    def forward(self, x, out=None, out_coff=0, stats_groups=None):
        if self.ks != (2, 2):
            assert out is None, "anisotropic transposed convolution writes its own tensor"
            y = self._forward_aniso(x)
            return (y, None) if stats_groups else y
        return self._packed(x, out, out_coff, stats_groups)


class GroupNorm(Module):
    """nn.GroupNorm(groups, C) (eps 1e-5) fused with the following activation / residual add.
    groups == C gives nn.InstanceNorm2d(C, affine=True) -- and, on an NCDHW tensor, nn.InstanceNorm3d: statistics over (D, H, W)."""

    def __init__(self, groups, channels, eps=1e-5):
        super().__init__()
        self.groups, self.eps = groups, eps
        self._param("weight", (channels,))
        self._param("bias", (channels,))

    def forward(self, x, act=None, res=None, res_mode=None, inplace=True, ws=None, res_norm=None):
        """ws: statistics already accumulated by the producing convolution's epilogue -> apply pass only.
        res_norm=(raw residual's statistics, its GroupNorm module): that norm is applied to `res` inside this pass.
        x (and res) NCDHW: the same pass on the [B, C, D*H, W] views."""
        if x.dim() == 5:
            B, C, D, H, W = x.shape
            y = self.forward(x.view(B, C, D * H, W), act, None if res is None else res.view(B, C, D * H, W), res_mode, inplace, ws, res_norm)
            return y.view(B, C, D, H, W)
        if res_norm is not None:
            ws_r, norm_r = res_norm
            if ws is not None and ws_r is not None and norm_r.groups == self.groups and norm_r.eps == self.eps:
                return ops.group_norm_apply(x, self._p["weight"], self._p["bias"], self.groups, ws, self.eps, act=act, res=res, res_mode=res_mode,
                                            out=x if inplace else None, res_norm=(ws_r, norm_r._p["weight"], norm_r._p["bias"]))
            res = norm_r(res, ws=ws_r)          # the branch's own pass (statistics not fused, or different group counts)
        if ws is not None:
            return ops.group_norm_apply(x, self._p["weight"], self._p["bias"], self.groups, ws, self.eps, act=act, res=res,
                                        res_mode=res_mode, out=x if inplace else None)
        return ops.group_norm(x, self._p["weight"], self._p["bias"], self.groups, self.eps, act=act, res=res, res_mode=res_mode,
                              out=x if inplace else None)


class InstanceNorm3d(GroupNorm):
    """nn.InstanceNorm3d(C, affine=True): GroupNorm with groups = C on the NCDHW tensor"""

    def __init__(self, channels, eps=1e-5):
        super().__init__(channels, channels, eps)


class BatchNorm(Module):
    """nn.BatchNorm2d / nn.BatchNorm3d(C, affine=True) in eval mode (nnUNetTrainerV2_BN): the [B, 3, C] table comes from the running
    statistics (ops.batch_norm_coef), one call per batch size, kept until the next load.  `groups` is None: the producing convolution is
    asked for no statistics.  `num_batches_tracked` is a derived buffer and never loaded."""
    groups = None

    def __init__(self, channels, eps=1e-5):
        super().__init__()
        self.eps = eps
        for k in ("weight", "bias", "running_mean", "running_var"):
            self._param(k, (channels,))
        self._tables = {}

    def _prepare(self):
        self._tables = {}

    def table(self, B):
        if B not in self._tables:
            p = self._p
            self._tables[B] = ops.batch_norm_coef(p["running_mean"], p["running_var"], p["weight"], p["bias"], B, self.eps)
        return self._tables[B]


class NoNorm(Module):
    """helperModules.Identity in the norm slot (nnUNetTrainerV2_NoNormalization): no parameters, no table -- the activation alone is applied"""
    groups = None

    def table(self, B):
        return None


def make_norm(kind, channels, groups=8, three_d=False):
    """the norm module of a Generic_UNet block: 'in' InstanceNorm(affine), 'gn' MyGroupNorm(groups), 'bn' BatchNorm (eval), 'none' Identity"""
    if kind == "in":
        return InstanceNorm3d(channels) if three_d else GroupNorm(channels, channels)
    if kind == "gn":
        return GroupNorm(groups, channels)
    if kind == "bn":
        return BatchNorm(channels)
    if kind == "none":
        return NoNorm()
    raise ValueError("norm must be 'in', 'gn', 'bn' or 'none', got %r" % (kind,))


class Nonlin(NamedTuple):
    """the activation of a Generic_UNet: kind 'lrelu' (with slope), 'relu', 'gelu' (erf form) or 'mish'"""
    kind: str = "lrelu"
    slope: float = 0.01

    @property
    def stage_slope(self):
        """what a consumer that normalises while staging takes for it (csrc/conv.h in_slope: v > 0 ? v : v * slope, negative: GELU);
        None: not deferrable (Mish)"""
        return {"lrelu": float(self.slope), "relu": 0.0, "gelu": -1.0}.get(self.kind)

    @property
    def fused(self):
        """its name among the fixed activations of the GroupNorm apply pass (LeakyReLU there is 0.01), or None: the pass is ops.coef_apply"""
        if self.kind == "lrelu":
            return "lrelu" if self.slope == 0.01 else None
        return self.kind if self.kind in ("relu", "gelu") else None

    def act_pass(self, x):
        """the activation alone, in place"""
        return ops.coef_apply(x, None, self.kind, self.slope, out=x)


LRELU = Nonlin()


class RawMap(NamedTuple):
    """a normalisation that has not run yet: a convolution's raw output, its statistics from the convolution's epilogue (None: not fused)
    and the norm module.  Whoever holds it applies the norm -- as a pass (`apply`, `norm_act`) or while staging the map (`coef`)."""
    raw: torch.Tensor
    ws: torch.Tensor
    norm: Module

    @property
    def ready(self):
        """can a consumer have the table without another pass over the map?  GroupNorm: the statistics came fused; BatchNorm: always;
        no norm: never (there is no table)"""
        return self.ws is not None if isinstance(self.norm, GroupNorm) else isinstance(self.norm, BatchNorm)

    def coef(self):
        """the [B, 3, C] table {mean, rstd * gamma, beta} a consumer that normalises while staging reads (None: no norm)"""
        B, C = self.raw.shape[:2]
        n = self.norm
        if not isinstance(n, GroupNorm):
            return n.table(B)
        ws = self.ws if self.ws is not None else ops.group_norm_stats(self.raw, n.groups)
        return ops.group_norm_coef(ws, n._p["weight"], n._p["bias"], n.groups, B, C, self.raw.numel() // (B * C), n.eps)

    def norm_act(self, nonlin=None):
        """nonlin(norm(raw)) as one pass, in place (nonlin None: the norm alone): the GroupNorm apply pass where its fixed activations cover
        `nonlin`, else ops.coef_apply on the table -- BatchNorm, no norm, LeakyReLU with another slope, Mish"""
        if isinstance(self.norm, GroupNorm) and (nonlin is None or nonlin.fused):
            return self.apply(None if nonlin is None else nonlin.fused)
        kind, slope = (None, 0.0) if nonlin is None else nonlin
        return ops.coef_apply(self.raw, self.coef(), kind, slope, out=self.raw)

    def apply(self, act=None, res=None, res_mode=None, inplace=True):
        """act(norm(raw)) with the residual inside the pass; a residual that is itself a RawMap gets its norm in the same pass"""
        if isinstance(res, RawMap):
            return self.norm(self.raw, act=act, res=res.raw, res_mode=res_mode, inplace=inplace, ws=self.ws, res_norm=(res.ws, res.norm))
        return self.norm(self.raw, act=act, res=res, res_mode=res_mode, inplace=inplace, ws=self.ws)


def conv_norm(conv, norm, x, x2=None, act=None, res=None, res_mode=None):
    """norm(conv(x)) with the GroupNorm statistics accumulated in the convolution's epilogue when possible; res as RawMap.apply's"""
    kw = {} if x2 is None else {"x2": x2}
    return RawMap(*conv(x, stats_groups=norm.groups, **kw), norm).apply(act, res, res_mode)


class LayerNormCF(Module):
    """nn.LayerNorm(C) applied over the channel axis of channel-first tokens."""

    def __init__(self, channels, eps=1e-5):
        super().__init__()
        self.eps = eps
        self._param("weight", (channels,))
        self._param("bias", (channels,))

    def forward(self, x, inplace=True):
        return ops.layer_norm_cf(x, self._p["weight"], self._p["bias"], self.eps, out=x if inplace else None)



# --------------------------------------------------------------------------------------------- 3-D layers
class Conv3d(Module):
    """nn.Conv3d for the 3-D U-Net behind _internal_predict_3D_3Dconv_tiled (generic_UNet.py with conv_op = nn.Conv3d).  Input/output NCDHW.
    (1|3, 3, 3) kernels run on the native kernel cf_conv3d_f16s (conv3d_f16s.hip) where ops.conv3d_f16s_ok takes the shape: one call on the
    NCDHW tensors, the InstanceNorm statistics of the output from its epilogue (stats_groups).  The (1, 1, 1) / stride-1 heads are a 1x1
    Conv2d on the [B, C, D*H, W] view.  A (1, 1, 1) kernel with a stride above 1 -- the skip projection of BasicResidualBlock3D -- runs
    on cf_conv3d_pw_f16s (conv3d_pw_f16s.hip) where ops.conv3d_pw_f16s_ok takes the shape, statistics likewise.
    Everything else -- its convroute.PackedConv3d answers None: set_conv_mode("f32"), one-term mode, declined shapes -- runs the composition:
    a (kd, k, k) convolution is the sum over the kd depth taps of 2-D (k, k) convolutions of depth-shifted planes, so it
    runs on the same MFMA implicit-GEMM kernels: the volume is re-laid as [B, D, C, H, W] planes, the centre tap writes
    every output plane (with the bias), the other taps accumulate through the kernel's residual input.  Kernel sizes 1 or 3
    per axis (padding 1 for 3, as generic_UNet.py:252-254), strides 1 or 2, equal in H and W."""

    def __init__(self, cin, cout, kernel_size=(3, 3, 3), stride=(1, 1, 1), bias=True):
        super().__init__()
        self.cin, self.cout, self.ks, self.stride = cin, cout, tuple(kernel_size), tuple(stride)
        assert all(k in (1, 3) for k in self.ks) and self.ks[1] == self.ks[2], "kernel sizes 1 or 3, equal in-plane"
        assert all(st in (1, 2) for st in self.stride) and self.stride[1] == self.stride[2], "strides 1 or 2, equal in-plane"
        self._param("weight", (cout, cin) + self.ks)
        if bias:
            self._param("bias", (cout,))

    def _prepare(self):
        if "weight" not in self._p:
            return
        pad = (self.ks[1] // 2, self.ks[1] // 2)
        if self.ks == (1, 1, 1) and self.stride == (1, 1, 1):
            # the segmentation heads: a 1x1 convolution on the [B, C, D*H, W] view of the NCDHW tensor, no re-layout
            self._head = Conv2d.from_tensors(self._p["weight"].reshape(self.cout, self.cin, 1, 1), self._p.get("bias"), self.cin, self.cout, 1)
            return
        self._packed = PackedConv3d(self._p["weight"], self._p.get("bias"), self.stride)      # the native and the pointwise kernel
        # the composed route: one 2-D convolution per depth tap (the layer's bias rides on the centre tap's call; never Winograd)
        self._taps = [PackedConv(self._p["weight"][:, :, dz].contiguous(), None, self.stride[1], pad) for dz in range(self.ks[0])]

    def forward(self, x, x2=None, stats_groups=None):
        """stats_groups=G: returns (out, ws) with the GroupNorm / InstanceNorm statistics of `out` when the native kernel ran, else (out, None)."""
        B, _, D, H, W = x.shape
        if hasattr(self, "_head"):
            assert x2 is None
            y = self._head(x.view(B, self.cin, D * H, W)).view(B, self.cout, D, H, W)
            return (y, None) if stats_groups else y
        y = self._packed(x, x2, stats_groups)
        if y is not None:
            return y
        y = self._forward_composed(x, x2)          # set_conv_mode("f32"), one-term mode and declined shapes
        return (y, None) if stats_groups else y

    def _forward_composed(self, x, x2=None):
        B, _, D, H, W = x.shape
        kd, sd, pd = self.ks[0], self.stride[0], self.ks[0] // 2
        k, st = self.ks[1], self.stride[1]
        Do = (D + 2 * pd - kd) // sd + 1
        Ho, Wo = (H + 2 * (k // 2) - k) // st + 1, (W + 2 * (k // 2) - k) // st + 1
        xp = x.permute(0, 2, 1, 3, 4).contiguous()
        x2p = None if x2 is None else x2.permute(0, 2, 1, 3, 4).contiguous()
        outp = torch.empty((B, Do, self.cout, Ho, Wo), dtype=torch.float32, device=x.device)
        bias = self._p.get("bias")
        order = [pd] + [dz for dz in range(kd) if dz != pd]          # centre tap first: it reaches every output plane
        for b in range(B):
            for n, dz in enumerate(order):
                zo_lo = max(0, -((dz - pd) // sd))                   # smallest zo with zo*sd + dz - pd >= 0
                zo_hi = min(Do - 1, (D - 1 - dz + pd) // sd)
                if zo_hi < zo_lo:
                    continue
                zi_lo = zo_lo * sd + dz - pd
                sl = slice(zi_lo, zi_lo + (zo_hi - zo_lo) * sd + 1, sd)
                xin = xp[b, sl] if sd == 1 else xp[b, sl].contiguous()
                xin2 = None if x2p is None else (x2p[b, sl] if sd == 1 else x2p[b, sl].contiguous())
                osl = outp[b, zo_lo:zo_hi + 1]
                self._taps[dz](xin, xin2, res=None if n == 0 else osl, out=osl, bias=bias if n == 0 else None)
        return outp.permute(0, 2, 1, 3, 4).contiguous()


class ConvTranspose3d(Module):
    """nn.ConvTranspose3d(kernel = stride = (kd, 2, 2), kd in {1, 2}, no overlap): output plane kd*z + dz is the 2-D transposed
    convolution of input plane z with the depth tap dz (generic_UNet.py:343-344 with the plans' pool_op_kernel_sizes)."""

    def __init__(self, cin, cout, kernel_size=(2, 2, 2), bias=False):
        super().__init__()
        self.cin, self.cout, self.ks = cin, cout, tuple(kernel_size)
        assert self.ks[0] in (1, 2) and self.ks[1:] == (2, 2), "transposed kernel (1|2, 2, 2)"
        self._param("weight", (cin, cout) + self.ks)
        if bias:
            self._param("bias", (cout,))

    def _prepare(self):
        if "weight" in self._p:
            self._taps = [PackedConvT(self._p["weight"][:, :, dz].contiguous(), self._p.get("bias")) for dz in range(self.ks[0])]    # [Cin,Cout,2,2] each

    def forward(self, x):
        B, C, D, H, W = x.shape
        kd = self.ks[0]
        xp = x.permute(0, 2, 1, 3, 4).contiguous().view(B * D, C, H, W)
        outp = torch.empty((B, D, kd, self.cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        for dz in range(kd):
            outp[:, :, dz] = self._taps[dz](xp).view(B, D, self.cout, 2 * H, 2 * W)
        return outp.view(B, D * kd, self.cout, 2 * H, 2 * W).permute(0, 2, 1, 3, 4).contiguous()


class BasicResidualBlock3D(Module):
    """custom_modules/conv_blocks.py:86-145 with conv_op = nn.Conv3d, InstanceNorm3d(affine), LeakyReLU(0.01), no dropout:
    lrelu(IN2(conv2(lrelu(IN1(conv1 x)))) + skip(x)), skip = identity or IN(conv1x1x1 at conv1's stride, no bias) -- the projection exists
    when any stride entry differs from 1 or cin != cout (:126).  The tail is ONE apply pass: IN2, the projection's own InstanceNorm (on
    its raw map, statistics from the projection's epilogue), the add and the LeakyReLU."""

    def __init__(self, cin, cout, kernel, stride=None):
        super().__init__()
        kernel = tuple(int(k) for k in kernel)
        st = (1, 1, 1) if stride is None else tuple(int(v) for v in stride)
        self.conv1 = Conv3d(cin, cout, kernel, st, bias=True)
        self.norm1 = InstanceNorm3d(cout)
        self.conv2 = Conv3d(cout, cout, kernel, (1, 1, 1), bias=True)
        self.norm2 = InstanceNorm3d(cout)
        self.has_skip = any(v != 1 for v in st) or cin != cout
        if self.has_skip:
            self.downsample_skip = {0: Conv3d(cin, cout, (1, 1, 1), st, bias=False), 1: InstanceNorm3d(cout)}

    def forward(self, x):
        t = conv_norm(self.conv1, self.norm1, x, act="lrelu")
        y = RawMap(*self.conv2(t, stats_groups=self.norm2.groups), self.norm2)
        res = x
        if self.has_skip:      # launched behind conv2 (profiles/layer_library_refactor.md pins the order; as conv_norm's argument it would lead)
            proj, norm = self.downsample_skip[0], self.downsample_skip[1]
            res = RawMap(*proj(x, stats_groups=norm.groups), norm)
        return y.apply("lrelu", res=res, res_mode="before_act")


class ResidualLayer3D(Module):
    """custom_modules/conv_blocks.py:214-227: num_blocks BasicResidualBlock3D, the first one strided and widening."""

    def __init__(self, cin, cout, kernel, num_blocks, first_stride=None):
        super().__init__()
        self.convs = [BasicResidualBlock3D(cin, cout, kernel, first_stride)] + [BasicResidualBlock3D(cout, cout, kernel) for _ in range(num_blocks - 1)]

    def forward(self, x):
        for b in self.convs:
            x = b(x)
        return x

# --------------------------------------------------------------------------------------------- lib/utils.py blocks

class DoubleConv(Module):
    """nnunet/lib/utils.py:1182-1215: GELU(GN(conv)) twice, residual (optionally 1x1 conv + GN) added after the
    second GELU.  `x2` is the second half of a channel concatenation (never materialised)."""

    def __init__(self, in_dim, out_dim, residual, stride=1, kernel_size=3):
        super().__init__()
        self.conv1 = Conv2d(in_dim, out_dim, kernel_size, stride=stride, padding=1)
        self.norm1 = GroupNorm(8, out_dim)
        self.conv2 = Conv2d(out_dim, out_dim, kernel_size, padding=1)
        self.norm2 = GroupNorm(8, out_dim)
        self.residual = residual
        self.has_ds = bool(residual and (in_dim != out_dim or stride != 1))
        if self.has_ds:
            self.downsample = {0: Conv2d(in_dim, out_dim, 1, stride=stride), 1: GroupNorm(8, out_dim)}

    def _stem_ok(self, x, x2):
        """conv1 and the 1x1 downsample convolution read the same few-channel input: one launch writes both raw maps (ops.stem_block)"""
        c1 = self.conv1
        return (x2 is None and self.has_ds and c1.sub is None and c1.stride == 1 and c1.cin <= 8 and c1.ks == (3, 3) and c1.pad == (1, 1)
                and self.downsample[1].groups == self.norm1.groups and ops.stem_block_ok(x, c1.cout, self.norm1.groups))

    def _shortcut(self, x, x2):
        """the 1x1 shortcut convolution's raw map (its GroupNorm rides in the block's final pass); None for a block without one"""
        if not self.has_ds:
            return None
        conv, norm = self.downsample[0], self.downsample[1]
        return RawMap(*conv(x, x2=x2, stats_groups=norm.groups), norm)

    def forward(self, x, x2=None, defer_last=None):
        """defer_last = the 3x3 head convolution that will consume this block's output alone (Decoder2D.final_conv): when it can form
        GELU(GN2(y2)) + GN_ds(r) itself while staging (ops.conv2d_small_cout_norm2), the final apply pass is left to it and the pending
        norms are handed on as the RawMaps (y2, r).  Returns x, or (x, pending) when defer_last is given (one of the two is None)."""
        short = ws_r = None          # ws_r alone: the stem's shortcut map was summed but not stored (the final pass rebuilds it from x)
        if self._stem_ok(x, x2):
            ds, dn = self.downsample[0], self.downsample[1]
            stem = (x, self.conv1._p["weight"], self.conv1._p.get("bias"), ds._p["weight"], ds._p.get("bias"), self.norm1.groups)
            if (defer_last is None and dn.groups == self.norm2.groups and dn.eps == self.norm2.eps
                    and ops.group_norm_apply_res_stem_ok(x, self.conv1.cout, self.norm2.groups)):
                t, ws1, ws_r = ops.stem_block_y(*stem)
            else:
                t, ws1, r, ws_s = ops.stem_block(*stem)
                short = RawMap(r, ws_s, dn)
        else:
            t, ws1 = self.conv1(x, x2=x2, stats_groups=self.norm1.groups)
        # conv2 applies GELU(GN1(t)) itself while it stages its input where it can, else norm1 runs as a pass.  The shortcut convolution
        # is launched behind a conv2 that took the norm and ahead of a plain one (the order profiles/layer_library_refactor.md pins).
        pre = ws1 is not None and self.conv2.prenorm_ok(t)
        if pre:
            y2 = RawMap(*self.conv2.prenorm(t, RawMap(t, ws1, self.norm1).coef(), -1.0, stats_groups=self.norm2.groups), self.norm2)
            short = short or (self._shortcut(x, x2) if ws_r is None else None)
        else:
            t = self.norm1(t, act="gelu", ws=ws1)
            short = short or (self._shortcut(x, x2) if ws_r is None else None)
            y2 = RawMap(*self.conv2(t, stats_groups=self.norm2.groups), self.norm2)
        if ws_r is not None:
            if y2.ws is not None:
                n2, ds, dn = self.norm2, self.downsample[0], self.downsample[1]
                return ops.group_norm_apply_res_stem(y2.raw, n2._p["weight"], n2._p["bias"], n2.groups, y2.ws, x, ds._p["weight"], ds._p.get("bias"), ws_r,
                                                     dn._p["weight"], dn._p["bias"], n2.eps, act="gelu", res_mode="after_act", out=y2.raw)
            short = self._shortcut(x, x2)          # conv2's statistics were not fused: the shortcut map is needed after all
        if (short is not None and defer_last is not None and pre and y2.ws is not None and short.ws is not None and defer_last.sub is None
                and ops.small_cout_norm2_ok(y2.raw, defer_last.cout, defer_last.ks[0], defer_last.ks[1], defer_last.stride, defer_last.pad)):
            return None, (y2, short)
        assert not self.residual or self.has_ds or x2 is None
        res = short if self.has_ds else x if self.residual else None          # added after the second GELU
        out = y2.apply("gelu", res=res, res_mode="after_act")
        return out if defer_last is None else (out, None)


class SingleConv(Module):
    """nnunet/lib/utils.py:1239-1264: residual (bare 1x1 conv) added before the GELU."""

    def __init__(self, in_dim, out_dim, residual, stride=1, kernel_size=3):
        super().__init__()
        self.conv1 = Conv2d(in_dim, out_dim, kernel_size, stride=stride, padding=1)
        self.norm1 = GroupNorm(8, out_dim)
        self.residual = residual
        self.has_ds = bool(residual and (in_dim != out_dim or stride != 1))
        if self.has_ds:
            self.downsample = Conv2d(in_dim, out_dim, 1, stride=stride)

    def forward(self, x, x2=None):
        if not self.residual:
            return conv_norm(self.conv1, self.norm1, x, x2=x2, act="gelu")
        r = self.downsample(x, x2=x2) if self.has_ds else x
        return conv_norm(self.conv1, self.norm1, x, x2=x2, act="gelu", res=r, res_mode="before_act")


class ConvBlocks2DGroupLegacy(Module):
    """nnunet/lib/utils.py:1345-1366 (widths rounded to multiples of 8 at :1349)."""

    def __init__(self, in_dim, out_dim, nb_blocks, stride=1, residual=False, kernel_size=3, nb_conv=2):
        super().__init__()
        dims = torch.linspace(in_dim, out_dim, nb_blocks + 1).int()
        dims[1:] = (torch.round(dims[1:] / 8) * 8).int()
        fn = DoubleConv if nb_conv == 2 else SingleConv
        self.blocks = [fn(in_dim=int(dims[i]), out_dim=int(dims[i + 1]), residual=residual, stride=stride) for i in range(nb_blocks)]

    def forward(self, x, x2=None, defer_last=None):
        """defer_last: DoubleConv.forward's, asked of the last block -> (x, pending)"""
        pending = None
        for i, b in enumerate(self.blocks):
            kw = {"x2": x2} if i == 0 else {}
            if defer_last is not None and i == len(self.blocks) - 1 and isinstance(b, DoubleConv):
                x, pending = b(x, defer_last=defer_last, **kw)
            else:
                x = b(x, **kw)
        return (x, pending) if defer_last is not None else x


class PatchExpand2DGroup(Module):
    """nnunet/lib/utils.py:1982-1994: ConvTranspose2d(k2,s2) + GroupNorm(8) + GELU."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.up = {0: ConvTranspose2d(in_dim, out_dim), 1: GroupNorm(8, out_dim)}

    def forward(self, x):
        return conv_norm(self.up[0], self.up[1], x, act="gelu")


class PatchMerging2DGroup(Module):
    """nnunet/lib/utils.py:2210-2229: conv3x3 stride 2 + GroupNorm(8) + GELU."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.reduction = {0: Conv2d(in_dim, out_dim, 3, stride=2, padding=1), 1: GroupNorm(8, out_dim)}

    def forward(self, x):
        return conv_norm(self.reduction[0], self.reduction[1], x, act="gelu")


# --------------------------------------------------------------------------------------------- encoder / decoder
class Encoder2D(Module):
    """nnunet/lib/encoder.py:541-660 (Encoder2D) and :689-801 (EncoderMotionAppearance, `motion_appearance=True`:
    returns (out_conv(x), x, skips))."""

    def __init__(self, d_model, conv_depth, in_dims, out_dims, nb_conv, extra_block, residual, downsample_conv,
                 motion_appearance=False):
        super().__init__()
        self.num_stages = len(conv_depth)
        self.extra_block, self.motion_appearance = extra_block, motion_appearance
        self.layers, self.downsample_layers = [], []
        out_dim = None
        for i in range(self.num_stages):
            out_dim = d_model if i == self.num_stages - 1 else in_dims[i + 1]
            self.layers.append(ConvBlocks2DGroupLegacy(in_dims[i], out_dims[i], conv_depth[i], residual=residual, nb_conv=nb_conv))
            if downsample_conv == 2:
                self.downsample_layers.append(
                    ConvBlocks2DGroupLegacy(out_dims[i], out_dim, 1, residual=residual, nb_conv=nb_conv, stride=2))
            else:
                self.downsample_layers.append(PatchMerging2DGroup(out_dims[i], out_dim))
        if extra_block or motion_appearance:
            self.out_conv = ConvBlocks2DGroupLegacy(out_dim, out_dim, conv_depth[-1], residual=residual, nb_conv=nb_conv)

    def forward(self, x):
        skips = []
        for layer, ds in zip(self.layers, self.downsample_layers):
            x = layer(x)
            skips.append(x)
            x = ds(x)
        if self.motion_appearance:
            return self.out_conv(x), x, skips
        if self.extra_block:
            x = self.out_conv(x)
        return x, skips


class Decoder2D(Module):
    """nnunet/lib/decoder_alt.py:807-923: per stage PatchExpand, cat(skip, x) (as a dual-input conv), conv block;
    final conv3x3 -> num_classes."""

    def __init__(self, d_model, conv_depth, in_encoder_dims, out_encoder_dims, num_classes, dot_multiplier, nb_conv, residual):
        super().__init__()
        assert dot_multiplier == 2
        self.num_stages = len(conv_depth)
        self.layers, self.upsample_layers = [], []
        for i in range(self.num_stages):
            in_dim = d_model if i == 0 else in_encoder_dims[i - 1]
            self.upsample_layers.append(PatchExpand2DGroup(in_dim, out_encoder_dims[i]))
            self.layers.append(ConvBlocks2DGroupLegacy(out_encoder_dims[i] * 2, out_encoder_dims[i], conv_depth[i], nb_conv=nb_conv,
                                                       residual=residual))
        self.final_conv = Conv2d(out_encoder_dims[-1], num_classes, 3, padding=1)

    def forward(self, x, skips):
        pending = None
        for i, (layer, up, skip) in enumerate(zip(self.layers, self.upsample_layers, reversed(skips))):
            if i == self.num_stages - 1:
                x, pending = layer(skip, x2=up(x), defer_last=self.final_conv)      # the head is the last block's only consumer
            else:
                x = layer(skip, x2=up(x))
        if pending is None:
            return self.final_conv(x)
        y2, r = pending
        return ops.conv2d_small_cout_norm2(y2.raw, y2.coef(), r.raw, r.coef(), self.final_conv._p["weight"], self.final_conv._p.get("bias"))


# --------------------------------------------------------------------------------------------- transformers
_pos_cache = {}


def position_embedding_sine_2d(H, W, C, device, temperature=10000.0, scale=2 * math.pi):
    """PositionEmbeddingSine2d(num_pos_feats=C/2, normalize=True), nnunet/lib/position_embedding.py:88-107.
    Input independent: computed once per (H, W, C) on the host and cached on the device as [1, C, H*W]."""
    key = (H, W, C, str(device))
    if key not in _pos_cache:
        npf = C // 2
        y_embed = torch.arange(1, H + 1, dtype=torch.float32)[:, None].expand(H, W)
        x_embed = torch.arange(1, W + 1, dtype=torch.float32)[None, :].expand(H, W)
        eps = 1e-6
        y_embed = y_embed / (y_embed[-1:, :] + eps) * scale
        x_embed = x_embed / (x_embed[:, -1:] + eps) * scale
        dim_t = torch.arange(npf, dtype=torch.float32)
        dim_t = temperature ** (2 * (dim_t // 2) / npf)
        pos_x = x_embed[:, :, None] / dim_t
        pos_y = y_embed[:, :, None] / dim_t
        pos_x = torch.stack((pos_x[:, :, 0::2].sin(), pos_x[:, :, 1::2].cos()), dim=3).flatten(2)
        pos_y = torch.stack((pos_y[:, :, 0::2].sin(), pos_y[:, :, 1::2].cos()), dim=3).flatten(2)
        pos = torch.cat((pos_y, pos_x), dim=2).permute(2, 0, 1).reshape(1, C, H * W).contiguous()
        _pos_cache[key] = pos.to(device)
    return _pos_cache[key]


class MultiheadAttention(Module):
    """nn.MultiheadAttention(d_model, nhead, batch_first=True) parameters; projections run as 1x1 convs on
    channel-first tokens, the core as cf_attention_cf."""

    def __init__(self, d_model, nhead):
        super().__init__()
        self.C, self.nhead = d_model, nhead
        self._param("in_proj_weight", (3 * d_model, d_model))
        self._param("in_proj_bias", (3 * d_model,))
        self.out_proj = _Linear(d_model, d_model)

    def _prepare(self):
        if "in_proj_weight" in self._p:
            C = self.C
            w, b = self._p["in_proj_weight"].view(3 * C, C, 1, 1), self._p["in_proj_bias"]
            self._q, self._k, self._v = (PackedConv(w[i * C:(i + 1) * C], b[i * C:(i + 1) * C]) for i in range(3))
            self._qk = PackedConv(w[:2 * C], b[:2 * C])          # q and k of one input in one launch (same_qk)

    def forward(self, q_in, k_in, v_in, residual, same_qk=False):
        """q_in [B,C,Nq,1], k_in/v_in [B,C,Nk,1]; returns residual + out_proj(attention)."""
        C = self.C
        B, _, Nq, _ = q_in.shape
        if same_qk:
            qk = self._qk(q_in)
            q, k = qk.view(B, 2 * C, Nq).narrow(1, 0, C), qk.view(B, 2 * C, Nq).narrow(1, C, C)
        else:
            q = self._q(q_in).view(B, C, Nq)
            k = self._k(k_in).view(B, C, -1)
        v = self._v(v_in).view(B, C, -1)
        att = ops.attention_cf(q, k, v, self.nhead).view(B, C, Nq, 1)
        return self.out_proj(att, res=residual)


class _Linear(Module):
    """nn.Linear on channel-first tokens [B,Cin,N,1] == 1x1 conv."""

    def __init__(self, cin, cout):
        super().__init__()
        self.cin, self.cout = cin, cout
        self._param("weight", (cout, cin))
        self._param("bias", (cout,))

    def _prepare(self):
        if "weight" in self._p:
            self._packed = PackedConv(self._p["weight"].view(self.cout, self.cin, 1, 1), self._p.get("bias"))

    def forward(self, x, act=None, res=None):
        return self._packed(x, act=act, res=res)


class TransformerFlowLayer(Module):
    """nnunet/lib/vit_transformer.py:1228-1270, post-norm: self-MHA(q=k=x+pos, v=x) -> LN -> cross-MHA(q=x+pos,
    k=key+pos, v=value) -> LN -> FFN(GELU) -> LN.  Residual adds are fused in the projection epilogues."""

    def __init__(self, d_model, nhead, dim_feedforward=2048):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead)
        self.cross_attn = MultiheadAttention(d_model, nhead)
        self.linear1 = _Linear(d_model, dim_feedforward)
        self.linear2 = _Linear(dim_feedforward, d_model)
        self.norm1, self.norm2, self.norm3 = LayerNormCF(d_model), LayerNormCF(d_model), LayerNormCF(d_model)

    def forward(self, query, key_pos_added, value, pos):
        """query, value [B,C,N,1]; key_pos_added = key + pos (precomputed by the caller); pos [1,C,N] broadcast."""
        B, C, N, _ = query.shape
        qp = ops.add(query, pos)
        x = self.self_attn(qp, qp, query, residual=query, same_qk=True)
        x = self.norm1(x.view(B, C, N)).view(B, C, N, 1)
        qp = ops.add(x, pos)
        x = self.cross_attn(qp, key_pos_added, value, residual=x)
        x = self.norm2(x.view(B, C, N)).view(B, C, N, 1)
        t = self.linear1(x, act="gelu")
        x = self.linear2(t, res=x)
        return self.norm3(x.view(B, C, N)).view(B, C, N, 1)


class CrossAttentionLayer(Module):
    """nnunet/lib/vit_transformer.py:5240-5287 ([B,C,H,W] in/out)."""

    def __init__(self, dim, nhead, num_layers, dim_feedforward):
        super().__init__()
        self.dim = dim
        self.bilateral_attention_layers = [TransformerFlowLayer(dim, nhead, dim_feedforward) for _ in range(num_layers)]

    def forward(self, query, key, value):
        B, C, H, W = query.shape
        pos = position_embedding_sine_2d(H, W, C, query.device)
        q = query.view(B, C, H * W, 1)
        kp = ops.add(key.view(B, C, H * W, 1), pos)
        v = value.view(B, C, H * W, 1)
        for layer in self.bilateral_attention_layers:
            q = layer(q, kp, v, pos)
        return q.view(B, C, H, W)


class TransformerFlowEncoderSuccessiveNoEmb(Module):
    """nnunet/lib/vit_transformer.py:3596-3641: the layer applied symmetrically to (forward, backward) adjacent
    frame pairs stacked on the batch axis.  Input [T,B,C,H,W] -> [T-1,B,C,H,W]."""

    def __init__(self, dim, nhead, num_layers):
        super().__init__()
        self.bilateral_attention_layers = [TransformerFlowLayer(dim, nhead) for _ in range(num_layers)]

    def forward(self, u):
        T, B, C, H, W = u.shape
        N = H * W
        pos = position_embedding_sine_2d(H, W, C, u.device)
        flat = u.reshape(T * B, C, N, 1)
        bwd = flat[:(T - 1) * B]
        fwd = flat[B:]
        for layer in self.bilateral_attention_layers:
            c0 = torch.cat([fwd, bwd], dim=0)  # pure copies (batch-axis concatenation)
            c1 = torch.cat([bwd, fwd], dim=0)
            c0 = layer(c0, ops.add(c1, pos), c1, pos)
            fwd, bwd = c0[:(T - 1) * B], c0[(T - 1) * B:]
        return fwd.reshape(T - 1, B, C, H, W)


# --------------------------------------------------------------------------------------------- ConvGRU, warp
class ConvGRUCell(Module):
    """nnunet/network_architecture/convGRU.py:7-69.  cat([x,h]) and cat([x,r*h]) are dual-input convs; sigmoid and
    tanh are conv epilogues."""

    def __init__(self, input_size, input_dim, hidden_dim, kernel_size=(3, 3), bias=True):
        super().__init__()
        self.height, self.width = input_size
        self.hidden_dim = hidden_dim
        pad = (kernel_size[0] // 2, kernel_size[1] // 2)
        self.conv_gates = Conv2d(input_dim + hidden_dim, 2 * hidden_dim, kernel_size, padding=pad, bias=bias)
        self.conv_can = Conv2d(input_dim + hidden_dim, hidden_dim, kernel_size, padding=pad, bias=bias)

    def forward(self, x, h):
        gates = self.conv_gates(x, x2=h, act="sigmoid")
        rh = ops.gru_reset_mul(gates, h)
        cand = self.conv_can(x, x2=rh, act="tanh")
        return ops.gru_blend(gates, h, cand)


class SpatialTransformer(Module):
    """nnunet/network_architecture/integration.py:37-79 (2-D and the 3-D branch :75-77, chosen by len(size)).  Keeps the
    reference's persistent `grid` buffer key so checkpoints load, but the kernel never reads it."""

    def __init__(self, size, mode="bilinear"):
        super().__init__()
        self.size = tuple(size)
        self.mode = mode

    def state_shapes(self, prefix=""):
        return {prefix + "grid": (1, len(self.size)) + self.size}

    def load_state_dict(self, sd, device, prefix="", strict=True):
        return self  # the identity grid is implicit in the kernel

    def forward(self, flow, original, mode="bilinear"):
        return ops.warp_bilinear(flow, original)


class VecInt(Module):
    """integration.py:82-99."""

    def __init__(self, inshape, nsteps):
        super().__init__()
        self.nsteps = nsteps
        self.transformer = SpatialTransformer(inshape)

    def forward(self, vec):
        return ops.vecint(vec, self.nsteps)
