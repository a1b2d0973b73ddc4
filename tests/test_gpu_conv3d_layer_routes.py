"""nn.Conv3d, nn.ConvTranspose3d and the anisotropic nn.ConvTranspose2d as layers, in the mode they ship in (set_conv_mode("f16s"), three-term
product), against fp64 references that share no code with the layers (tests/_conv3d_layer_refs.py, checked on the CPU by
test_split_exact_reference.py).

Conv3d.  cf_conv3d_f16s_ok leaves four classes of shape to the composition of 2-D convolutions -- composition_is_faster (a), (b), (c) of
csrc/conv3d_f16s.hip and the shapes geometry() has no tile for -- and those are the largest and the deepest layers of a 3d_fullres plan.  Rows
1 to 10 and 12 are such shapes (the declined side of the probe pairs test_reference_import_3d.py asks on the host), row 11 is row 1's
neighbour on the native kernel.  Each row builds the layer, calls it once and asserts
    route       the real probe declines the row and takes its neighbour, no knob is set, and spies see exactly one _forward_composed whose
                taps all ran on ops.conv2d_f16s -- none on ops.conv2d, which would be a second fallback passing (native row: one
                ops.conv3d_f16s, nothing composed);
    call order  per sample the centre tap first, with the layer's bias and no residual, then the other in-range taps with res aliasing out
                and no bias; each call's input is the planes that tap reads, its output the planes it reaches (enumerated plane by plane
                in in_range_taps, not with nn.py's closed forms); the 2-D plan of each call is the kernel shape the row is there for;
    value       |out - y3| <= 2^-18 A everywhere (worst ratio printed, pytest -s), and the same output FAILS that bar against y3 without the
                last input channel, without depth tap 0 and one plane off along depth; 1e-5 against the fp64 convolution of the true operands;
    input       bit-identical after the call;
    statistics  stats_groups = Cout: fp64-checked statistics from the native kernel, None from the composition.
The composed rows run again under set_conv_mode("f32"): the same indexing on the exact fp32 kernel, at 1e-5.

Row 9 found a bug: a 130x1 map has no 3-D geometry, and the 2-D plan declined its taps too ("staging tasks exceed MAXT"), so the layer
raised in the default mode.  f16s_plan now gives such a tile fewer rows; the 2-D table (test_gpu_conv_f16s_routes.py NARROW_ROWS) holds
the new tiles to the split-exact bar on their own.

Transposed layers.  F.conv_transpose3d / F.conv_transpose2d on the split operands, one scale per depth tap; the output fails the bar
without the last input channel and with the two interleaved positions exchanged (depth taps, sub-rows, sub-columns).

Network.  Generic_UNet3D on 4x128x128, two kernel plans: the (1,3,3) layers at full resolution are class (a) and compose (stage 0; in the
second plan the last decoder stage too, with the skip as x2), everything between runs native, so RawMap.ws alternates between None and
fused statistics; logits against the fp64 oracle at the network's 1e-4.
"""
import inspect

import pytest
import torch

from _conv3d_layer_refs import (LAYER_ROWS, PAIR, T_ROWS, TAP_NIMG, host_scales, in_range_taps, layer_operands, layer_reference, lrow_id,
                                probe_args, shifted, t_host_scales, t_operands, t_reference, t_swaps, trow_id)
from _split_exact import SPLIT_BAR, check_stats, randn, ratio

pytestmark = pytest.mark.gpu

COMPOSED_ROWS = [r for r in LAYER_ROWS if r.pair != "native"]
SPIED = ("conv2d_f16s", "conv2d", "conv2d_wino", "conv2d_small_cin", "conv2d_small_cout", "conv3d_f16s", "conv3d_pw_f16s",
         "conv_transpose2d_k2s2_f16s", "conv_transpose2d_k2s2")


def spy_on(monkeypatch):
    """log of (name, {argument: value}) for every convolution entry point of ops and ("composed", {"self": layer}) for the composition"""
    from cineflow import nn as PN, ops
    log = []

    def wrap(name, real):
        sig = inspect.signature(real)

        def spied(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            log.append((name, dict(bound.arguments)))
            return real(*a, **k)
        return spied
    for name in SPIED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    real_composed = PN.Conv3d._forward_composed
    monkeypatch.setattr(PN.Conv3d, "_forward_composed", lambda self, *a, **k: log.append(("composed", {"self": self})) or real_composed(self, *a, **k))
    return log


def calls_of(log, name):
    return [args for n, args in log if n == name]


def probe(t):
    from cineflow import ops
    return ops.conv3d_f16s_ok(*t[:7], (t[7], t[8], t[8]), (t[9], t[10], t[10]))


def build_layer(row, dev):
    from cineflow.nn import Conv3d
    x, w, b = layer_operands(row)
    m = Conv3d(row.C1 + row.C2, row.Cout, row.k, row.stride, bias=True)
    m.load_state_dict({"weight": w, "bias": b}, dev)
    xd = x.to(dev)
    return m, xd[:, :row.C1].contiguous(), (xd[:, row.C1:].contiguous() if row.C2 else None)


def out_dims(row):
    kd, k = row.k[0], row.k[1]
    sd, st = row.stride[0], row.stride[1]
    return (row.D + 2 * (kd // 2) - kd) // sd + 1, (row.H + 2 * (k // 2) - k) // st + 1, (row.W + 2 * (k // 2) - k) // st + 1


def split_key_of(row, tap):
    return row.C1 if (row.C2 and row.C1 % tap.chunk) else None


def check_tap_calls(row, m, calls, x1d, x2d, f16s):
    """the call-order assertions of the module docstring on the calls of ops.conv2d_f16s (f16s) or ops.conv2d"""
    want = in_range_taps(row)
    assert len(calls) == len(want), (len(calls), len(want))
    k, st, pd = row.k[1], row.stride[1], row.k[0] // 2
    Do, Ho, Wo = out_dims(row)
    plane = row.Cout * Ho * Wo * 4
    base = calls[0]["out"].data_ptr()          # sample 0, centre tap: it reaches output plane 0
    for c, (b, dz, zo, zi) in zip(calls, want):
        tap, what = m._taps[dz], (row.n, b, dz)
        if f16s:
            key = split_key_of(row, tap)
            assert key in tap._pk, what
            assert c["wpk"].data_ptr() == tap._pk[key][0].data_ptr() and c["wscale"] == tap._pk[key][1], what
        else:
            assert c["wt"].data_ptr() == tap.wt.data_ptr(), what
        assert (c["kh"], c["kw"], c["stride"], tuple(c["pad"]), c["cout"]) == (k, k, st, (k // 2, k // 2), row.Cout), what
        assert c["act"] is None and c["alpha"] == 1.0 and c["out_coff"] == 0, what
        out = c["out"]
        assert out.data_ptr() == base + (b * Do + zo) * plane and tuple(out.shape) == (len(zi), row.Cout, Ho, Wo) and out.is_contiguous(), what
        if dz == pd:
            assert c["bias"] is not None and c["bias"].data_ptr() == m._p["bias"].data_ptr() and c["res"] is None, what
        else:
            assert c["bias"] is None, what
            assert c["res"] is not None and c["res"].data_ptr() == out.data_ptr() and c["res"].shape == out.shape, what
        idx = torch.tensor(zi, device=x1d.device)
        assert c["x1"].is_contiguous() and torch.equal(c["x1"], x1d[b].index_select(1, idx).permute(1, 0, 2, 3)), what
        if x2d is None:
            assert c["x2"] is None, what
        else:
            assert c["x2"].is_contiguous() and torch.equal(c["x2"], x2d[b].index_select(1, idx).permute(1, 0, 2, 3)), what


def check_values(name, o, ref, kd, D):
    """the value assertions on an fp64 copy of the device output; returns the worst ratio to the bar"""
    bar = SPLIT_BAR * ref["A"]
    worst = ratio(o, ref["y3"], bar)
    print("\n%s worst |out - y3| / (2^-18 A) = %.4f" % (name, worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    if kd == 3:
        if D > 1:
            assert ratio(o, ref["y3"] - ref["z3"], bar) > 1.0, "a dropped depth tap dz = 0 would pass the bar"
        else:
            assert float(ref["z3"].abs().max()) == 0.0
    if o.dim() == 5 and o.shape[2] > 1:
        assert ratio(o, shifted(ref["y3"]), bar) > 1.0, "planes one off along depth would pass the bar"
    d = float((o - ref["true"]).abs().max())
    assert d <= 1e-5, ("fp64 contract", d)
    return worst


@pytest.mark.parametrize("row", LAYER_ROWS, ids=lrow_id)
def test_conv3d_layer_route(dev, row, monkeypatch):
    from cineflow import _lib, ops
    assert ops.CONV_MODE == "f16s" and _lib.lib().cf_conv_terms(3) == 3, "a knob is forcing the route"
    native = row.pair == "native"
    if native:
        assert probe_args(row) == PAIR["a"][1] and probe(probe_args(row)), "the probe declines the native row"
    elif row.pair is None:
        assert not probe(probe_args(row))                       # 1x1 taps: no native kernel has the shape
    else:
        declined, taken = PAIR[row.pair]
        assert probe_args(row) == declined
        assert not probe(declined) and probe(taken), "the row is not on the declined side of its probe pair"
    m, x1d, x2d = build_layer(row, dev)
    keep1, keep2 = x1d.clone(), (None if x2d is None else x2d.clone())
    log = spy_on(monkeypatch)
    out, ws = m(x1d, x2d, stats_groups=row.Cout)
    torch.cuda.synchronize()
    assert torch.equal(x1d, keep1) and (x2d is None or torch.equal(x2d, keep2)), "the layer wrote its input"
    names = [n for n, _ in log]
    if native:
        assert names == ["conv3d_f16s"], names
        scales = (m._packed._pk[None][1],) * row.k[0]
        check_stats(out.cpu(), ws, row.B, row.Cout, list(range(row.B)))
        plan_txt = "native cf_conv3d_f16s"
    else:
        assert names.count("composed") == 1 and log[0][1]["self"] is m, names
        taps = calls_of(log, "conv2d_f16s")
        assert len(taps) == len(names) - 1, ("a tap left conv2d_f16s", names)
        check_tap_calls(row, m, taps, x1d, x2d, f16s=True)
        assert ws is None
        scales = tuple(t.packed(split_key_of(row, t))[1] for t in m._taps)
        plans = []
        for c in taps:
            plan = ops.conv2d_f16s_route(c["x1"], row.Cout, c["kh"], c["kw"], c["stride"], c["pad"], x2=c["x2"])
            assert plan.route in (1, 2) and plan.terms == 3 and plan.part == c["x1"].shape[0], plan
            assert plan.nimg == TAP_NIMG.get(row.n, {}).get(c["x1"].shape[0], 1), (plan, c["x1"].shape)
            plans.append(plan)
        plan_txt = "composed, %d tap calls, first %s" % (len(taps), plans[0])
    assert scales == host_scales(row, layer_operands(row)[1])
    ref = layer_reference(row, scales)
    assert tuple(out.shape) == tuple(ref["y3"].shape)
    print("\n%s %s" % (lrow_id(row), plan_txt), end="")
    check_values(lrow_id(row), out.cpu().double(), ref, row.k[0], row.D)


@pytest.mark.parametrize("row", COMPOSED_ROWS, ids=lrow_id)
def test_conv3d_layer_fp32_mode(dev, row, monkeypatch):
    """the same layers under set_conv_mode("f32"): every tap on the exact fp32 kernel, the same slices, 1e-5 against fp64"""
    from cineflow import ops
    m, x1d, x2d = build_layer(row, dev)
    keep1 = x1d.clone()
    log = spy_on(monkeypatch)
    ops.set_conv_mode("f32")
    try:
        out, ws = m(x1d, x2d, stats_groups=row.Cout)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_mode("f16s")
    names = [n for n, _ in log]
    assert names.count("composed") == 1 and ws is None and torch.equal(x1d, keep1)
    taps = calls_of(log, "conv2d")
    assert len(taps) == len(names) - 1, names
    check_tap_calls(row, m, taps, x1d, x2d, f16s=False)
    want = layer_reference(row, host_scales(row, layer_operands(row)[1]))["true"]
    d = float((out.cpu().double() - want).abs().max())
    print("\n%s fp32 mode max|out - fp64| = %.2e" % (lrow_id(row), d))
    assert d <= 1e-5, d


@pytest.mark.parametrize("row", T_ROWS, ids=trow_id)
def test_transposed_layer(dev, row, monkeypatch):
    from cineflow import ops
    from cineflow.nn import ConvTranspose2d, ConvTranspose3d
    assert ops.CONV_MODE == "f16s"
    x, w, b = t_operands(row)
    m = ConvTranspose3d(row.C, row.Cout, row.k, bias=row.bias) if row.dims == 3 else ConvTranspose2d(row.C, row.Cout, bias=row.bias, kernel_size=row.k)
    m.load_state_dict({"weight": w, "bias": b} if row.bias else {"weight": w}, dev)
    xd = x.to(dev)
    keep = xd.clone()
    log = spy_on(monkeypatch)
    out = m(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
    names = [n for n, _ in log]
    if row.dims == 3:
        D, H, W = row.size
        assert names == ["conv_transpose2d_k2s2_f16s"] * row.k[0], names
        for dz, c in enumerate(calls_of(log, "conv_transpose2d_k2s2_f16s")):
            assert tuple(c["x"].shape) == (row.B * D, row.C, H, W) and c["wpk"].data_ptr() == m._taps[dz].wpk.data_ptr()
            assert (c["bias"] is not None) == row.bias and c["wscale"] == m._taps[dz].scale
        scales = tuple(t.scale for t in m._taps)
    else:
        # the anisotropic layers are a 1x1 convolution to Cout * 2 GEMM rows and a strided copy: the f16-split 2-D kernel, not the scatter
        assert names == ["conv2d_f16s"], names
        scales = (m._w1._packed.scale,)
    assert scales == t_host_scales(row, w)
    ref = t_reference(row, scales)
    assert tuple(out.shape) == tuple(ref["y3"].shape)
    o = out.cpu().double()
    check_values(trow_id(row), o, ref, 0, 0)
    bar = SPLIT_BAR * ref["A"]
    for name, y in t_swaps(row, ref["y3"]).items():
        assert ratio(o, y, bar) > 1.0, "exchanged %s would pass the bar" % name


POOL3 = [[1, 2, 2], [2, 2, 2]]
# the net of test_gpu_unet3d_native.py, and the same with (1,3,3) kernels in stage 1 as well: the last decoder stage takes
# conv_kernel_sizes[-2] (generic_UNet.py), so only the second net has class (a) layers there
NETS = {"k133_333_333": ([[1, 3, 3], [3, 3, 3], [3, 3, 3]], 2), "k133_133_333": ([[1, 3, 3], [1, 3, 3], [3, 3, 3]], 4)}


@pytest.mark.parametrize("name", list(NETS))
def test_unet3d_alternates_composed_and_native_layers(dev, monkeypatch, name):
    """Generic_UNet3D(1, 4, 3, 2) on a 1x1x4x128x128 input.  The (1,3,3) layers at full resolution have 65536 output voxels and no depth
    taps (class (a)): both stage-0 convolutions compose and the next layer runs native, so consecutive InstanceNorms get None and fused
    statistics.  In the second net the last decoder stage is (1,3,3) too: its two convolutions compose after six native layers, the first
    with the skip as x2.  Logits against oracle.models.GenericUNet3D in float64 at the network's 1e-4.  Should that fail with every layer
    row green, the message carries the all-native 4x64x64 figure (the input's top-left quarter) to tell the routes apart."""
    from cineflow import ops
    from cineflow.models import Generic_UNet3D
    from cineflow.weights import fill_module_, seeded_state_dict
    from oracle import models as OM
    kern, ncomposed = NETS[name]
    net = Generic_UNet3D(1, 4, 3, 2, pool_op_kernel_sizes=POOL3, conv_kernel_sizes=kern)
    net.load_state_dict(seeded_state_dict(net.state_shapes(), 20), dev)
    ora = fill_module_(OM.GenericUNet3D(1, 4, 3, 2, pool_op_kernel_sizes=POOL3, conv_kernel_sizes=kern), 20).double()
    x = randn(1, 1, 4, 128, 128, seed=77)
    assert ops.CONV_MODE == "f16s"
    ctx, loc = net.conv_blocks_context, net.conv_blocks_localization
    want_composed = [ctx[0].blocks[0].conv, ctx[0].blocks[1].conv, loc[1][0].blocks[0].conv, loc[1][1].blocks[0].conv][:ncomposed]
    assert all(c.ks == (1, 3, 3) for c in want_composed)

    def run(inp):
        with monkeypatch.context() as mp:
            log = spy_on(mp)
            y = net(inp.to(dev))
            torch.cuda.synchronize()
        with torch.no_grad():
            return log, float((y.cpu().double() - ora(inp.double())).abs().max())

    log, d = run(x)
    composed = [a["self"] for n, a in log if n == "composed"]
    assert len(composed) == ncomposed and all(a is b for a, b in zip(composed, want_composed)), [c.ks for c in composed]
    native = calls_of(log, "conv3d_f16s")
    assert len(native) == 10 - ncomposed and not calls_of(log, "conv2d"), [n for n, _ in log]
    # the routes alternate in the order of the forward: stage 0 composed, six native layers, then the decoder's composed pair
    order = [n for n, _ in log if n in ("composed", "conv3d_f16s")]
    assert order == ["composed"] * 2 + ["conv3d_f16s"] * 6 + (["composed"] * 2 if ncomposed == 4 else ["conv3d_f16s"] * 2), order
    taps = [a for n, a in log if n == "conv2d_f16s" and a["kh"] == 3]
    assert [a["x2"] is not None for a in taps] == [False, False, True, False][:ncomposed]
    print("\nGeneric_UNet3D %s 4x128x128, %d composed + %d native layers: logits max|diff| = %.3e (bar 1e-4)" % (name, ncomposed, 10 - ncomposed, d))
    if d > 1e-4:
        log_q, d_q = run(x[..., :64, :64].contiguous())
        assert not [n for n, _ in log_q if n == "composed"]
        pytest.fail("logits max|diff| %.3e > 1e-4; all-native 4x64x64 quarter: %.3e" % (d, d_q))
