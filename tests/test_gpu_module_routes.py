"""Which kernel family every convolution-bearing module class sends a call to, and that the module computes exactly what the direct
`ops.*` call of that route computes on weights from the public packers (bit equality: a single convolution without statistics-dependent
inputs is deterministic).  One row per module class and route; every row runs under set_conv_mode("f16s") and once more under "f32",
where no f16 or Winograd launch may appear and the fp32 MFMA kernel carries every launch -- the stems and the flow heads included.
Families are told apart by the launch counters of cf_profile_read: fp32 implicit GEMM with one / two m-tiles (ids 0 / 1: Cout <= 32 / wider;
the transposed convolution's GEMM has 4 * Cout rows), conv_f16s (6), the direct small-Cout kernel (14), conv_stream (15), conv_wino (16);
the direct small-Cin kernel has no counter (its row expects zero everywhere).  Shapes are at most 2 x 256 x 16 x 32.
Fused statistics are checked with check_stats at its 2e-6 bar, not bit for bit (their atomics meet in any order).
The last test reloads a mtl.Sequential with other weights: its folded conv + BatchNorm layer must follow the reload."""
import contextlib
import ctypes

import pytest
import torch

from _split_exact import check_stats, randn

pytestmark = pytest.mark.gpu

FAMILIES = {"mt1": 0, "mt2": 1, "f16s": 6, "small_cout": 14, "stream": 15, "wino": 16}


@contextlib.contextmanager
def wino_forced(level):
    from cineflow._lib import lib
    prev = lib().cf_conv_wino_enable(level)
    try:
        yield
    finally:
        lib().cf_conv_wino_enable(prev)


@contextlib.contextmanager
def launch_counts():
    """{family: launches} of the convolution families for the calls made inside (filled on exit)"""
    from cineflow._lib import check, lib
    h = lib()
    got = {}
    check(h.cf_profile_enable(64), "cf_profile_enable")
    try:
        yield got
        torch.cuda.synchronize()
        for name, kid in FAMILIES.items():
            ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
            check(h.cf_profile_read(kid, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)), "cf_profile_read")
            got[name] = n.value
    finally:
        check(h.cf_profile_enable(0), "cf_profile_enable")


def loaded(m, dev, seed):
    """the module with seeded weights on the device, and those weights"""
    from cineflow.weights import seeded_state_dict
    sd = {k: v.to(dev) for k, v in seeded_state_dict(m.state_shapes(), seed).items()}
    m.load_state_dict(sd, dev)
    return m, sd


def direct(mode, x, w, b, stride=1, pad=(0, 0), c1=None, **kw):
    """the direct ops call of a mode's MFMA route: conv2d_f16s on pack_conv_weight_f16s' tensor, or conv2d on the transposed matrix"""
    from cineflow import ops
    cout, _, kh, kw_ = w.shape
    if mode == "f32":
        return ops.conv2d(x, ops.prep_conv_weight(w), b, cout, kh, kw_, stride, pad, **kw)
    wpk, s = ops.pack_conv_weight_f16s(w, c1=c1)
    return ops.conv2d_f16s(x, wpk, s, b, cout, kh, kw_, stride, pad, **kw)


def direct_t(mode, x, w, b, **kw):
    from cineflow import ops
    cin, cout = w.shape[:2]
    if mode == "f32":
        return ops.conv_transpose2d_k2s2(x, w, b, **kw)
    wpk, s = ops.pack_conv_weight_f16s(w.permute(1, 2, 3, 0).reshape(cout * 4, cin, 1, 1))
    return ops.conv_transpose2d_k2s2_f16s(x, wpk, s, b, cout, **kw)


# Every row: (dev, mode) -> (launch counts of the module call, expected counts {family: n} (others 0), [(module output, direct output)]).
def conv_row(cin, cout, k, pad, shape, f16s_family, f32_family, x2_channels=0, wino=None, direct_f16s=None, **call):
    def row(dev, mode):
        from cineflow import ops
        from cineflow.nn import Conv2d
        m, sd = loaded(Conv2d(cin + x2_channels, cout, k, padding=pad), dev, 7)
        w, b = sd["weight"], sd["bias"]
        x = randn(shape[0], cin, *shape[1:], seed=1).to(dev)
        kw = dict(call)
        if x2_channels:
            kw["x2"] = randn(shape[0], x2_channels, *shape[1:], seed=2).to(dev)
        with wino_forced(wino) if wino is not None else contextlib.nullcontext():
            with launch_counts() as n:
                y = m(x, **kw)
            if mode == "f16s" and f16s_family == "wino":
                ref = ops.conv2d_wino(x, *ops.pack_conv_weight_wino(w), b, cout, **kw)
            elif mode == "f16s" and direct_f16s is not None:
                ref = getattr(ops, direct_f16s)(x, w, b)
            else:
                ref = direct("f32" if f16s_family in ("mt1", "mt2") else mode, x, w, b, 1, (pad, pad), c1=cin if x2_channels else None, **kw)
        return n, ({f16s_family: 1} if f16s_family else {}) if mode == "f16s" else {f32_family: 1}, [(y, ref)]
    return row


def linear_row(dev, mode):
    from cineflow.nn import _Linear
    m, sd = loaded(_Linear(256, 256), dev, 8)
    x, res = randn(2, 256, 64, 1, seed=3).to(dev), randn(2, 256, 64, 1, seed=4).to(dev)
    with launch_counts() as n:
        y = m(x, act="gelu", res=res)
    return n, {"f16s" if mode == "f16s" else "mt2": 1}, [(y, direct(mode, x, sd["weight"].view(256, 256, 1, 1), sd["bias"], act="gelu", res=res))]


def attention_row(dev, mode):
    from cineflow import ops
    from cineflow.nn import MultiheadAttention
    C, N = 256, 64
    m, sd = loaded(MultiheadAttention(C, 4), dev, 9)
    w, b = sd["in_proj_weight"].view(3 * C, C, 1, 1), sd["in_proj_bias"]
    qp, x = randn(2, C, N, 1, seed=5).to(dev), randn(2, C, N, 1, seed=6).to(dev)
    with launch_counts() as n:
        y = m(qp, qp, x, residual=x, same_qk=True)
    qk = direct(mode, qp, w[:2 * C].contiguous(), b[:2 * C].contiguous()).view(2, 2 * C, N)
    v = direct(mode, x, w[2 * C:].contiguous(), b[2 * C:].contiguous()).view(2, C, N)
    att = ops.attention_cf(qk.narrow(1, 0, C), qk.narrow(1, C, C), v, 4).view(2, C, N, 1)
    ref = direct(mode, att, sd["out_proj.weight"].view(C, C, 1, 1), sd["out_proj.bias"], res=x)
    return n, {"f16s" if mode == "f16s" else "mt2": 3}, [(y, ref)]          # qk, v, out_proj


def conv_transpose_row(dev, mode):
    from cineflow.nn import ConvTranspose2d
    m, sd = loaded(ConvTranspose2d(32, 16), dev, 10)
    x = randn(2, 32, 8, 8, seed=7).to(dev)
    with launch_counts() as n:
        y, st = m(x, stats_groups=8)
    if mode == "f16s":
        check_stats(y.cpu(), st, 2, 8, [0, 1])
    else:
        assert st is None
    return n, {"f16s" if mode == "f16s" else "mt2": 1}, [(y, direct_t(mode, x, sd["weight"], sd["bias"]))]


def conv_transpose_aniso_row(dev, mode):
    from cineflow.nn import ConvTranspose2d
    m, sd = loaded(ConvTranspose2d(32, 16, kernel_size=(2, 1)), dev, 11)
    x = randn(2, 32, 8, 8, seed=8).to(dev)
    with launch_counts() as n:
        y = m(x)
    w1 = sd["weight"].permute(1, 2, 3, 0).reshape(32, 32, 1, 1).contiguous()          # the inner 1x1 layer: rows co * 2 + dy
    ref = direct(mode, x, w1, sd["bias"].repeat_interleave(2).contiguous()).view(2, 16, 2, 1, 8, 8)
    ref = ref.permute(0, 1, 4, 2, 5, 3).reshape(2, 16, 16, 8).contiguous()
    return n, {"f16s" if mode == "f16s" else "mt1": 1}, [(y, ref)]


def conv3d_composed_row(dev, mode):
    """one-term mode keeps the layer off the native 3-D kernel: one 2-D launch per in-range (depth tap, sample), the centre tap first (it
    carries the bias), the others accumulating through the residual input; never Winograd"""
    from cineflow import ops
    from cineflow.nn import Conv3d
    m, sd = loaded(Conv3d(8, 16, (3, 3, 3)), dev, 12)
    x = randn(1, 8, 4, 16, 16, seed=9).to(dev)
    with ops.conv_terms(1):
        with launch_counts() as n:
            y = m(x)
        planes = x.permute(0, 2, 1, 3, 4).contiguous()[0]          # [D, C, H, W]
        ref = torch.empty((4, 16, 16, 16), dtype=torch.float32, device=dev)
        for i, (dz, zo, zi) in enumerate(((1, slice(0, 4), slice(0, 4)), (0, slice(1, 4), slice(0, 3)), (2, slice(0, 3), slice(1, 4)))):
            direct(mode, planes[zi], sd["weight"][:, :, dz].contiguous(), sd["bias"] if i == 0 else None, 1, (1, 1),
                   res=None if i == 0 else ref[zo], out=ref[zo])
    return n, {"f16s" if mode == "f16s" else "mt1": 3}, [(y, ref.permute(1, 0, 2, 3)[None].contiguous())]


def conv3d_head_row(dev, mode):
    from cineflow.nn import Conv3d
    m, sd = loaded(Conv3d(8, 4, (1, 1, 1), bias=False), dev, 13)
    x = randn(1, 8, 4, 16, 16, seed=10).to(dev)
    with launch_counts() as n:
        y = m(x)
    ref = direct(mode, x.view(1, 8, 64, 16), sd["weight"].reshape(4, 8, 1, 1), None).view(1, 4, 4, 16, 16)
    return n, {"f16s" if mode == "f16s" else "mt1": 1}, [(y, ref)]


def conv_transpose3d_row(dev, mode):
    from cineflow.nn import ConvTranspose3d
    m, sd = loaded(ConvTranspose3d(16, 8, (2, 2, 2)), dev, 14)
    x = randn(1, 16, 2, 8, 8, seed=11).to(dev)
    with launch_counts() as n:
        y = m(x)
    planes = x.permute(0, 2, 1, 3, 4).contiguous().view(2, 16, 8, 8)
    ref = torch.stack([direct_t(mode, planes, sd["weight"][:, :, dz].contiguous(), None) for dz in range(2)], 1)      # [D, kd, Cout, 16, 16]
    return n, {"f16s" if mode == "f16s" else "mt1": 2}, [(y, ref.reshape(4, 8, 16, 16).permute(1, 0, 2, 3)[None].contiguous())]


def sepconvgru_row(dev, mode):
    from cineflow import ops
    from cineflow.models import SepConvGRU
    m, sd = loaded(SepConvGRU(128, 256), dev, 15)
    h, x = randn(1, 128, 16, 16, seed=12).to(dev), randn(1, 256, 16, 16, seed=13).to(dev)
    with launch_counts() as n:
        y = m(h, x)
    ref = h
    for p, pad in (("1", (0, 2)), ("2", (2, 0))):
        wrz = torch.cat([sd["convr%s.weight" % p], sd["convz%s.weight" % p]]).contiguous()
        brz = torch.cat([sd["convr%s.bias" % p], sd["convz%s.bias" % p]]).contiguous()
        gates = direct(mode, ref, wrz, brz, 1, pad, x2=x, act="sigmoid")
        q = direct(mode, ops.gru_reset_mul(gates, ref), sd["convq%s.weight" % p], sd["convq%s.bias" % p], 1, pad, x2=x, act="tanh")
        ref = ops.gru_blend(gates, ref, q)
    return n, {"f16s" if mode == "f16s" else "mt2": 4}, [(y, ref)]


def mask_head_row(dev, mode):
    """BasicUpdateBlock with its encoder, GRU and flow head stubbed out: the two convolutions of the mask head alone, the second one with
    alpha = 0.25 and the 0.25-scaled bias.  Winograd is off so that the first one's family is known (conv_f16s)."""
    from cineflow.models import BasicUpdateBlock
    m, sd = loaded(BasicUpdateBlock(hidden_dim=128), dev, 16)
    m.encoder, m.gru, m.flow_head = (lambda flow, corr, out: out), (lambda net, inp: net), (lambda net: None)
    net = randn(1, 128, 16, 16, seed=14).to(dev)
    with wino_forced(0):
        with launch_counts() as n:
            _, mask, _ = m(net, None, None, None)
        hidden = direct(mode, net, sd["mask.0.weight"], sd["mask.0.bias"], 1, (1, 1), act="relu")
    ref = direct(mode, hidden, sd["mask.2.weight"], (0.25 * sd["mask.2.bias"]).contiguous(), alpha=0.25)
    return n, {"f16s" if mode == "f16s" else "mt2": 2}, [(mask, ref)]


ROWS = {
    "conv_wino": conv_row(64, 128, 3, 1, (2, 16, 32), "wino", "mt2", wino=1),
    "conv_w48": conv_row(64, 128, 3, 1, (2, 16, 48), "f16s", "mt2", wino=1),                  # W = 48: no Winograd tile
    "conv_split_20_28": conv_row(20, 64, 3, 1, (2, 16, 32), "f16s", "mt2", x2_channels=28),    # split-aware packing, c1 = 20
    "conv_flow_head": conv_row(64, 2, 3, 1, (2, 16, 32), "small_cout", "mt1", direct_f16s="conv2d_small_cout"),
    "conv_flow_head_relu": conv_row(64, 2, 3, 1, (2, 16, 32), "f16s", "mt1", act="relu"),       # an activation: not the direct kernel's
    "conv_stem": conv_row(1, 32, 3, 1, (2, 16, 32), None, "mt1", direct_f16s="conv2d_small_cin"),
    "conv_7x7": conv_row(2, 32, 7, 3, (2, 16, 32), "mt1", "mt1"),                                # no f16 kernel shape
    "linear": linear_row,
    "attention_same_qk": attention_row,
    "conv_transpose": conv_transpose_row,
    "conv_transpose_2x1": conv_transpose_aniso_row,
    "conv3d_composed": conv3d_composed_row,
    "conv3d_head": conv3d_head_row,
    "conv_transpose3d": conv_transpose3d_row,
    "sepconvgru": sepconvgru_row,
    "mask_head": mask_head_row,
}


@pytest.mark.parametrize("mode", ["f16s", "f32"])
@pytest.mark.parametrize("row", list(ROWS))
def test_module_route(dev, row, mode):
    from cineflow import ops
    prev = ops.CONV_MODE
    ops.set_conv_mode(mode)
    try:
        n, expected, pairs = ROWS[row](dev, mode)
    finally:
        ops.set_conv_mode(prev)
    assert n == {**dict.fromkeys(FAMILIES, 0), **expected}, n
    if mode == "f32":
        assert n["f16s"] == n["wino"] == n["stream"] == n["small_cout"] == 0
    for got, want in pairs:
        assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())


def test_sequential_reload_drops_the_folded_layers(dev):
    """a mtl.Sequential loaded a second time computes with the second checkpoint: the conv + BatchNorm layer it folded for the first one
    must not survive the reload"""
    from cineflow import mtl
    from cineflow.nn import Conv2d
    from cineflow.weights import seeded_state_dict

    def load(s, seed):
        return s.load_state_dict(seeded_state_dict(s.state_shapes(), seed), dev)

    def fresh():
        return mtl.Sequential({0: Conv2d(8, 8, 3, padding=1), 1: mtl.BatchNorm2d(8)})
    x = randn(2, 8, 16, 16, seed=20).to(dev)
    s = load(fresh(), 1)
    ya = s.conv_bn(0, x).clone()
    yb = load(s, 2).conv_bn(0, x)
    assert torch.equal(yb, load(fresh(), 2).conv_bn(0, x))
    assert float((yb - ya).abs().max()) > 1e-2
