"""Generic_UNet3D on the native 3-D convolution kernel (csrc/conv3d_f16s.hip): the golden 3-D network of test_gpu_models.py must run every
(1|3,3,3) convolution through cf_conv3d_f16s, keep its bars against the REFERENCE's outputs (logits 1e-4, tiled softmax 2e-5), and keep them on
the fallback composition under set_conv_mode("f32")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

POOL3, KERN3 = [[1, 2, 2], [2, 2, 2]], [[1, 3, 3], [3, 3, 3], [3, 3, 3]]


def _maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(np.asarray(b)).double()).abs().max())


@pytest.fixture(scope="module")
def net(dev):
    from cineflow.models import Generic_UNet3D
    from cineflow.weights import seeded_state_dict
    m = Generic_UNet3D(1, 4, 3, 2, pool_op_kernel_sizes=POOL3, conv_kernel_sizes=KERN3)
    m.load_state_dict(seeded_state_dict(m.state_shapes(), 20), dev)
    return m


def _convs(mod):
    from cineflow.nn import Conv3d
    if isinstance(mod, Conv3d):
        yield mod
    for _, child in mod._children():
        yield from _convs(child)


def test_every_spatial_conv3d_runs_native_and_matches_the_reference(dev, golden, net, monkeypatch):
    from cineflow import nn as PN, ops
    from cineflow.inference import predict_3D_3Dconv_tiled
    g = golden("generic_unet_3d")
    x = torch.from_numpy(g["x"]).to(dev)
    spatial = [c for c in _convs(net) if c.ks != (1, 1, 1)]
    assert len(spatial) == 10 and len(list(_convs(net))) == 12          # 3 encoder + 2 decoder stages x 2 convolutions; 2 heads
    asked, composed = [], []
    real_ok, real_comp = ops.conv3d_f16s_ok, PN.Conv3d._forward_composed
    monkeypatch.setattr(ops, "conv3d_f16s_ok", lambda *a: asked.append((a, real_ok(*a))) or asked[-1][1])
    monkeypatch.setattr(PN.Conv3d, "_forward_composed", lambda self, *a: composed.append(self.ks) or real_comp(self, *a))
    logits = net(x)
    assert len(asked) == len(spatial) and all(ok for _, ok in asked), [a for a, ok in asked if not ok]
    assert not composed, composed
    d = _maxdiff(logits, g["logits"])
    assert d <= 1e-4, "Generic_UNet 3-D logits max|diff| %.3e" % d
    seg, prob = predict_3D_3Dconv_tiled(net, g["vol"], (8, 16, 16), 0.5, True, (0, 1, 2), True, "constant", {"constant_values": 0})
    assert not composed
    d = _maxdiff(prob, g["tiled_prob"])
    assert d <= 2e-5, "tiled softmax max|diff| %.3e" % d


def test_fp32_mode_keeps_the_composition(dev, golden, net, monkeypatch):
    from cineflow import nn as PN, ops
    g = golden("generic_unet_3d")
    composed = []
    real_comp = PN.Conv3d._forward_composed
    monkeypatch.setattr(PN.Conv3d, "_forward_composed", lambda self, *a: composed.append(self.ks) or real_comp(self, *a))
    ops.set_conv_mode("f32")
    try:
        d = _maxdiff(net(torch.from_numpy(g["x"]).to(dev)), g["logits"])
    finally:
        ops.set_conv_mode("f16s")
    assert len(composed) == 10
    assert d <= 1e-4, "fp32 mode max|diff| %.3e" % d


def test_one_term_mode_keeps_the_composition(dev, net):
    """only the three-term product is built: under conv_terms(1) the probe answers 0 and the layer stays on the 2-D composition"""
    from cineflow import ops
    assert ops.conv3d_f16s_ok(1, 4, 0, 8, 16, 16, 4, (3, 3, 3), (1, 1, 1))
    with ops.conv_terms(1):
        assert not ops.conv3d_f16s_ok(1, 4, 0, 8, 16, 16, 4, (3, 3, 3), (1, 1, 1))


def test_111_head_is_a_1x1_convolution_on_the_plane_view(dev):
    from cineflow.nn import Conv3d
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 3, 10, 12, generator=gen)
    w = torch.randn(4, 8, 1, 1, 1, generator=gen) / 8 ** 0.5
    m = Conv3d(8, 4, (1, 1, 1), bias=False)
    m.load_state_dict({"weight": w}, dev)
    want = F.conv3d(x.double(), w.double())
    d = _maxdiff(m(x.to(dev)), want)
    assert d <= 1e-5, d
