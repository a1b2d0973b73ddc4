"""cf_conv2d_small_cout_norm2: the 3x3 flow head that forms its input GELU(GN2(y2)) + GN_ds(r) while staging, against the two launches it
replaces (the DoubleConv's final apply pass, then cf_conv2d_small_cout).

The convolution's FMA order over (ci, co, ky, kx) is the replaced kernel's, but the value a tap sees is not bit-identical: the coefficient table
of cf_group_norm_coef holds the ROUNDED product rstd * gamma, where the apply pass multiplies by rstd and by gamma one after the other (an ulp
of the normalised value).  So the bar is the one tests/test_gpu_ops.py holds conv3x3_small_cout to: 2e-5 (fp32 accumulation over 9 * Cin terms)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS = 8


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def stats(t):
    """{sum, sum of squares} per (sample, group) in fp64, as the convolutions' fused statistics hold them"""
    B = t.shape[0]
    d = t.double().view(B, GROUPS, -1)
    return torch.stack([d.sum(-1), (d ** 2).sum(-1)], -1).reshape(-1).contiguous()


@pytest.mark.parametrize("B,H,W", [(2, 8, 12), (3, 8, 12), (2, 33, 20), (3, 33, 20)])
def test_flow_head_forms_its_input(dev, B, H, W):
    from cineflow import ops
    C, K = 64, 2
    y2 = (randn(B, C, H, W, seed=400) * 1.5 + 0.3).to(dev)
    r = (randn(B, C, H, W, seed=401) * 0.7 - 0.2).to(dev)
    g2, b2, gr, br = (t.to(dev) for t in (1.0 + 0.3 * randn(C, seed=402), 0.2 * randn(C, seed=403), 1.0 + 0.3 * randn(C, seed=404), 0.2 * randn(C, seed=405)))
    w = (randn(K, C, 3, 3, seed=406) / math.sqrt(9 * C)).to(dev)
    bias = randn(K, seed=407).to(dev)
    ws2, wsr = stats(y2), stats(r)
    x = ops.group_norm_apply(y2, g2, b2, GROUPS, ws2, act="gelu", res=r, res_mode="after_act", res_norm=(wsr, gr, br), out=torch.empty_like(y2))
    want = ops.conv2d_small_cout(x, w, bias)
    assert ops.small_cout_norm2_ok(y2, K, 3, 3, 1, (1, 1))
    c2 = ops.group_norm_coef(ws2, g2, b2, GROUPS, B, C, H * W)
    cr = ops.group_norm_coef(wsr, gr, br, GROUPS, B, C, H * W)
    got = ops.conv2d_small_cout_norm2(y2, c2, r, cr, w, bias)
    torch.cuda.synchronize()
    d = float((got - want).abs().max())
    print("\nflow head B %d %dx%d: max|fused - two launches| %.2e (bar 2e-5; outputs up to %.2f)" % (B, H, W, d, float(want.abs().max())))
    assert got.shape == (B, K, H, W) and d <= 2e-5
    # no bias; and a NaN in sample 1's residual map stays in sample 1
    assert float((ops.conv2d_small_cout_norm2(y2, c2, r, cr, w, None) - ops.conv2d_small_cout(x, w, None)).abs().max()) <= 2e-5
    rn = r.clone()
    rn[1, 5, 3, 4] = float("nan")
    gn = ops.conv2d_small_cout_norm2(y2, c2, rn, cr, w, bias)
    assert torch.equal(gn[0], got[0]) and torch.isnan(gn[1]).any()


def test_flow_head_probe_and_decoder_route(dev):
    """the probe declines more than four output channels, and Decoder2D leaves its last apply pass to the head exactly when the probe accepts"""
    from cineflow import ops
    from cineflow.nn import Decoder2D
    from cineflow.weights import seeded_state_dict
    y = torch.empty(2, 8, 16, 16, device=dev)
    assert ops.small_cout_norm2_ok(y, 2, 3, 3, 1, (1, 1)) and not ops.small_cout_norm2_ok(y, 8, 3, 3, 1, (1, 1)) and not ops.small_cout_norm2_ok(y, 2, 1, 1, 1, (0, 0))
    m = Decoder2D(d_model=32, dot_multiplier=2, conv_depth=[1, 1, 1], in_encoder_dims=[32, 16, 4], out_encoder_dims=[32, 16, 8], num_classes=2, nb_conv=2,
                  residual=True)
    m.load_state_dict(seeded_state_dict(m.state_shapes(), 7), dev)
    xb = randn(2, 32, 8, 8, seed=1).to(dev)
    skips = [randn(2, 8, 64, 64, seed=2).to(dev), randn(2, 16, 32, 32, seed=3).to(dev), randn(2, 32, 16, 16, seed=4).to(dev)]
    seen = []
    real = ops.conv2d_small_cout_norm2
    ops.conv2d_small_cout_norm2 = lambda *a: (seen.append(1), real(*a))[1]
    try:
        fused = m(xb, skips)
        assert len(seen) == 1
        ok = ops.small_cout_norm2_ok
        ops.small_cout_norm2_ok = lambda *a: False
        try:
            plain = m(xb, skips)
        finally:
            ops.small_cout_norm2_ok = ok
        assert len(seen) == 1
    finally:
        ops.conv2d_small_cout_norm2 = real
    d = float((fused - plain).abs().max())
    print("\nDecoder2D: fused head vs apply pass + head: max|diff| %.2e (bar 2e-5)" % d)
    assert fused.shape == (2, 2, 64, 64) and d <= 2e-5
