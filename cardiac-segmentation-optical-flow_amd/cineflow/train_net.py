"""The training twin of models.Generic_UNet (2-D): a forward pass that keeps what the backward needs, and the backward itself.

Same constructor arguments and parameter names as models.Generic_UNet (generic_UNet.py:167-408 as nnUNetTrainerV2.py:147-169 builds it:
InstanceNorm affine, LeakyReLU 0.01, strided first convolutions, bias-free transposed convolutions and heads, deep supervision on).  The
forward runs the exact-fp32 operators with no deferred norm -- ops.conv2d, ops.conv_transpose2d_k2s2, ops.group_norm_stats /
group_norm_apply -- and records, per layer, its inputs, raw map and statistics.  backward() walks that list in reverse with the kernels of
train_ops; it is a list of records of three kinds, not an autograd.

Master weights live in one flat fp32 arena in the layout the forward reads ([(Cin*kh*kw), Cout] for convolutions, torch's own for
transposed convolutions); gradients and momentum buffers in two arenas of the same shape.  wgrad writes that layout and the optimizer steps
in it; state_dict() converts to the reference's layout, and only there."""
import collections

import numpy as np
import torch

from . import ops
from . import train_ops as T

MAX_FILTERS_2D = 480


def check_servable(plans):
    """Refuse, by key, every plans.json choice the training path does not serve."""
    if plans.get("flow_net"):
        raise ValueError("flow_net: the flow trainers are not served by cineflow.train (segmentation-only training)")
    if plans.get("regions") or plans.get("regions_class_order"):
        raise ValueError("regions: region-based training (sigmoid heads) is not served by cineflow.train")
    sk = plans.get("seg_net") or {}
    if int(sk.get("dim", 2)) != 2:
        raise ValueError("seg_net.dim = %r: cineflow.train serves the 2-D Generic_UNet only" % (sk.get("dim"),))
    for key in ("regions", "prev_stage_classes", "arch"):
        if sk.get(key) is not None:
            raise ValueError("seg_net.%s = %r is not served by cineflow.train (plain 2-D Generic_UNet only)" % (key, sk[key]))
    check_variant(**{k: sk[k] for k in ("norm", "nonlin", "block_order", "nonlin_slope") if k in sk})


def check_variant(norm="in", nonlin="lrelu", block_order="conv_norm_nonlin", nonlin_slope=0.01, **other):
    if norm != "in":
        raise ValueError("seg_net.norm = %r: cineflow.train serves 'in' (InstanceNorm) only" % (norm,))
    if nonlin != "lrelu" or float(nonlin_slope) != 0.01:
        raise ValueError("seg_net.nonlin = %r (slope %r): cineflow.train serves 'lrelu' with slope 0.01 only" % (nonlin, nonlin_slope))
    if block_order != "conv_norm_nonlin":
        raise ValueError("seg_net.block_order = %r: cineflow.train serves 'conv_norm_nonlin' only" % (block_order,))
    for k in other:
        if k != "norm_groups":
            raise ValueError("seg_net.%s is not served by cineflow.train" % k)


def deep_supervision_weights(num_pool):
    """nnUNetTrainerV2_noDA.py:72-77: 1 / 2**i per output, the lowest resolution zeroed, normalised."""
    w = np.array([1 / (2 ** i) for i in range(num_pool)])
    w[-1] = 0
    return w / w.sum()


def deep_supervision_scales(pool_op_kernel_sizes):
    """nnUNetTrainerV2.py:111-112: the target scale of every output, full resolution first"""
    return [[1, 1]] + [list(v) for v in 1 / np.cumprod(np.vstack(pool_op_kernel_sizes), axis=0)][:-1]


class TrainNet(object):
    def __init__(self, input_channels, base_num_features, num_classes, num_pool, num_conv_per_stage=2, pool_op_kernel_sizes=None,
                 seg_output_bias=False, **variant):
        check_variant(**variant)
        pool = [tuple(int(v) for v in p_) for p_ in (pool_op_kernel_sizes or [(2, 2)] * num_pool)]
        if len(pool) != num_pool or any(p_ not in ((2, 2), (2, 1), (1, 2)) for p_ in pool):
            raise ValueError("pool_op_kernel_sizes: (2,2), (2,1) or (1,2), one per stage")
        self.input_channels, self.num_classes, self.num_pool, self.pool = input_channels, num_classes, num_pool, pool
        self.seg_output_bias = bool(seg_output_bias)
        # ---- the layer plan: stacks of (name, cin, cout, stride) blocks
        self.ctx, self.loc, self.tu, self.seg = [], [], [], []
        shapes = collections.OrderedDict()        # reference layout

        def stack(prefix, cin, cout, n, first_stride=None):
            blocks = []
            for i in range(n):
                name = "%s.blocks.%d" % (prefix, i)
                blocks.append((name, cin if i == 0 else cout, cout, (first_stride or (1, 1)) if i == 0 else (1, 1)))
                shapes[name + ".conv.weight"] = (cout, cin if i == 0 else cout, 3, 3)
                shapes[name + ".conv.bias"] = (cout,)
                shapes[name + ".instnorm.weight"] = (cout,)
                shapes[name + ".instnorm.bias"] = (cout,)
            return blocks

        out_f, in_f = base_num_features, input_channels
        skip_ch = []
        for d in range(num_pool):
            self.ctx.append(stack("conv_blocks_context.%d" % d, in_f, out_f, num_conv_per_stage, pool[d - 1] if d else None))
            skip_ch.append(out_f)
            in_f = out_f
            out_f = min(int(np.round(out_f * 2)), MAX_FILTERS_2D)
        final = out_f
        self.ctx.append(stack("conv_blocks_context.%d.0" % num_pool, in_f, out_f, num_conv_per_stage - 1, pool[-1]) +
                        stack("conv_blocks_context.%d.1" % num_pool, out_f, final, 1))
        for u in range(num_pool):
            from_down, from_skip = final, skip_ch[-(1 + u)]
            final = from_skip
            self.tu.append(("tu.%d" % u, from_down, from_skip, pool[-(u + 1)]))
            shapes["tu.%d.weight" % u] = (from_down, from_skip) + pool[-(u + 1)]
            self.loc.append(stack("conv_blocks_localization.%d.0" % u, from_skip * 2, from_skip, num_conv_per_stage - 1) +
                            stack("conv_blocks_localization.%d.1" % u, from_skip, final, 1))
            self.seg.append(("seg_outputs.%d" % u, final, num_classes))
            shapes["seg_outputs.%d.weight" % u] = (num_classes, final, 1, 1)
            if self.seg_output_bias:
                shapes["seg_outputs.%d.bias" % u] = (num_classes,)
        self.shapes = shapes
        self.names = list(shapes)
        self.offsets, off = {}, 0
        for n, s in shapes.items():
            self.offsets[n] = (off, int(np.prod(s)))
            off += (int(np.prod(s)) + 3) & ~3            # every tensor starts on 16 bytes
        self.arena_size = off
        self.device = None
        self.records = None
        self._tables = {}

    def state_shapes(self):
        return collections.OrderedDict(self.shapes)

    # ---- arenas ---------------------------------------------------------------------------------------------------------------------------
    def _master_shape(self, name):
        s = self.shapes[name]
        if len(s) == 4 and not name.startswith("tu."):
            return (s[1] * s[2] * s[3], s[0])
        return s

    def _views(self, arena):
        return {n: arena[o:o + sz].view(self._master_shape(n)) for n, (o, sz) in self.offsets.items()}

    def to(self, device):
        self.device = torch.device(device)
        self.param = torch.zeros(self.arena_size, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros_like(self.param)
        self.mom = torch.zeros_like(self.param)
        self.p, self.g = self._views(self.param), self._views(self.grad)
        self._tables = {}
        return self

    def _to_master(self, name, t):
        t = t.detach().to(torch.float32)
        if t.dim() == 4 and not name.startswith("tu."):
            return t.reshape(t.shape[0], -1).t()
        return t

    def _from_master(self, name, t):
        s = self.shapes[name]
        if len(s) == 4 and not name.startswith("tu."):
            return t.t().reshape(s)
        return t.reshape(s)

    def load_state_dict(self, sd, device=None):
        """sd: {name: tensor} in the reference's layout (a Generic_UNet state_dict)"""
        if device is not None or self.device is None:
            self.to(device if device is not None else "cuda:0")
        missing = [n for n in self.names if n not in sd]
        if missing:
            raise KeyError("state dict lacks %s" % missing[:4])
        for n in self.names:
            if tuple(sd[n].shape) != tuple(self.shapes[n]):
                raise ValueError("%s: shape %s, expected %s" % (n, tuple(sd[n].shape), self.shapes[n]))
            self.p[n].copy_(self._to_master(n, sd[n]))
        return self

    def _layout(self, views):
        return collections.OrderedDict((n, self._from_master(n, views[n]).contiguous().cpu()) for n in self.names)

    def state_dict(self):
        return self._layout(self.p)

    def grad_dict(self):
        return self._layout(self.g)

    def init_weights(self, seed=0, neg_slope=1e-2):
        """InitWeights_He(1e-2) (initialization.py): kaiming_normal_(a = 1e-2) on every convolution and transposed convolution, biases 0;
        InstanceNorm affine at torch's defaults (1, 0)."""
        gen = torch.Generator().manual_seed(int(seed))
        sd = {}
        for n, s in self.shapes.items():
            if len(s) == 4:
                fan_in = s[1] * s[2] * s[3]
                std = np.sqrt(2.0 / (1 + neg_slope ** 2)) / np.sqrt(fan_in)
                sd[n] = torch.randn(s, generator=gen) * std
            else:
                sd[n] = torch.ones(s) if n.endswith("instnorm.weight") else torch.zeros(s)
        return self.load_state_dict(sd, self.device)

    def table(self, no_grad=()):
        """device int64 [T, 3] = {offset, size, has_grad} in parameter order"""
        key = tuple(sorted(no_grad))
        if key not in self._tables:
            rows = [[self.offsets[n][0], self.offsets[n][1], 0 if n in no_grad else 1] for n in self.names]
            self._tables[key] = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return self._tables[key]

    @property
    def max_tensor(self):
        return max(sz for _o, sz in self.offsets.values())

    # ---- forward --------------------------------------------------------------------------------------------------------------------------
    def _block(self, blk, x1, x2=None):
        name, _cin, cout, stride = blk
        w, b = self.p[name + ".conv.weight"], self.p[name + ".conv.bias"]
        if stride[0] == stride[1]:
            y, full = ops.conv2d(x1, w, b, cout, 3, 3, stride=stride[0], pad=(1, 1), x2=x2), None
        else:                                            # a per-axis stride runs as inference runs it: stride 1, then subsampling
            y1 = ops.conv2d(x1, w, b, cout, 3, 3, stride=1, pad=(1, 1), x2=x2)
            y, full = T.subsample(y1, stride), tuple(y1.shape[2:])
        ws = ops.group_norm_stats(y, cout)
        a = ops.group_norm_apply(y, self.p[name + ".instnorm.weight"], self.p[name + ".instnorm.bias"], cout, ws, act="lrelu")
        self.records.append(("block", name, x1, x2, y, ws, stride, full, a))
        return a

    def forward_train(self, x):
        """x [B, Cin, H, W] on the device -> [full-resolution logits, then every coarser decoder stage's head] (deep supervision)"""
        assert x.is_cuda and x.dtype == torch.float32 and x.shape[1] == self.input_channels
        self.records = []
        self._input = x
        skips = []
        for d in range(self.num_pool):
            for blk in self.ctx[d]:
                x = self._block(blk, x)
            skips.append(x)
        for blk in self.ctx[-1]:
            x = self._block(blk, x)
        heads = []
        for u in range(self.num_pool):
            name = self.tu[u][0]
            up = T.conv_transpose_fwd(x, self.p[name + ".weight"])
            self.records.append(("up", name, x, up))
            x = up
            for i, blk in enumerate(self.loc[u]):
                x = self._block(blk, x, skips[-(u + 1)] if i == 0 else None)
            hname, _c, K = self.seg[u]
            logits = ops.conv2d(x, self.p[hname + ".weight"], self.p.get(hname + ".bias"), K, 1, 1)
            self.records.append(("head", hname, x, logits))
            heads.append(logits)
        return heads[::-1]

    # ---- backward -------------------------------------------------------------------------------------------------------------------------
    def backward(self, dlogits):
        """dlogits: one tensor per output of forward_train (None: that output is not supervised -- its head gets no gradient).  Fills the
        gradient arena; returns the names of the parameters WITHOUT a gradient (torch's `grad is None`)."""
        assert self.records is not None and len(dlogits) == self.num_pool
        dl = {self.seg[u][0]: d for u, d in enumerate(dlogits[::-1])}
        grads = {}                                       # id(activation) -> its gradient; a second gradient is added to the first, in walk order

        def slot(t):
            g = grads.get(id(t))
            if g is None:
                g = grads[id(t)] = torch.empty_like(t)
                return g, False
            return g, True

        no_grad = set()
        for rec in reversed(self.records):
            kind, name = rec[0], rec[1]
            if kind == "head":
                _k, _n, x, logits = rec
                d = dl[name]
                if d is None:
                    no_grad.update(n for n in (name + ".weight", name + ".bias") if n in self.shapes)
                    continue
                assert d.shape == logits.shape
                has_b = name + ".bias" in self.g
                T.conv2d_wgrad(x, d, 1, want_bias=has_b, dw=self.g[name + ".weight"], db=self.g.get(name + ".bias"))
                g, acc = slot(x)
                T.conv2d_dgrad(d, self.p[name + ".weight"], tuple(x.shape[2:]), 1, dx=g, accumulate=acc)
            elif kind == "up":
                _k, _n, x, up = rec
                g, acc = slot(x)
                T.conv_transpose_bwd(x, self.p[name + ".weight"], grads.pop(id(up)), dw=self.g[name + ".weight"], dx=g, accumulate=acc)
            else:
                _k, _n, x1, x2, y, ws, stride, full, a = rec
                d = grads.pop(id(a))
                draw, _dg, _db = T.norm_act_bwd(y, d, ws, self.p[name + ".instnorm.weight"], self.p[name + ".instnorm.bias"],
                                                dgamma=self.g[name + ".instnorm.weight"], dbeta=self.g[name + ".instnorm.bias"])
                s = stride[0]
                if full is not None:
                    draw, s = T.scatter_stride(draw, full, stride), 1
                w = self.p[name + ".conv.weight"]
                T.conv2d_wgrad(x1, draw, 3, stride=s, x2=x2, want_bias=True, dw=self.g[name + ".conv.weight"], db=self.g[name + ".conv.bias"])
                C1 = x1.shape[1]
                if x1 is not self._input:
                    g, acc = slot(x1)
                    T.conv2d_dgrad(draw, w, tuple(x1.shape[2:]), 3, stride=s, ci_off=0, cn=C1, dx=g, accumulate=acc)
                if x2 is not None:
                    g, acc = slot(x2)
                    T.conv2d_dgrad(draw, w, tuple(x2.shape[2:]), 3, stride=s, ci_off=C1, cn=x2.shape[1], dx=g, accumulate=acc)
        self.records = None
        return no_grad
