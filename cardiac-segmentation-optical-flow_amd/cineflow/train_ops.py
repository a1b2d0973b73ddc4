"""Tensor-level wrappers over the training entry points of the C ABI (include/cineflow.h, "training"): the backward of ops.conv2d and of
InstanceNorm + LeakyReLU, the deep-supervision DC + CE loss, gradient clipping and Nesterov SGD.

As in ops.py, torch provides device memory, views and the current stream; every number comes from a HIP kernel.  The compositions below
(transposed convolutions, per-axis strides) move data with torch views and copies only -- no torch arithmetic."""
import torch

from ._lib import lib, check
from .ops import _f32, _opt, _stream

SLOPE = 0.01
EPS = 1e-5


def _out_hw(H, W, k, stride):
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def wgrad_splits(cin, cout, k, B, Ho, Wo):
    """the number of pixel chunks conv2d_wgrad cuts this shape into (a function of the shape alone)"""
    n = lib().cf_conv2d_wgrad_splits(cin, cout, k, k, B, Ho, Wo)
    check(min(n, 0), "cf_conv2d_wgrad_splits")
    return n


def conv2d_wgrad(x1, dy, k, stride=1, x2=None, want_bias=False, dw=None, db=None):
    """(dW [(C1+C2)*k*k, Cout] in ops.conv2d's layout, db [Cout] or None) of conv(cat[x1, x2]) with a k x k kernel, pad k // 2."""
    B, C1, H, W = x1.shape
    C2 = 0 if x2 is None else x2.shape[1]
    if x2 is not None:
        assert x2.shape[0] == B and x2.shape[2:] == x1.shape[2:]
    cout = dy.shape[1]
    Ho, Wo = _out_hw(H, W, k, stride)
    assert dy.shape == (B, cout, Ho, Wo), (dy.shape, (B, cout, Ho, Wo))
    ktot = (C1 + C2) * k * k
    splits = wgrad_splits(C1 + C2, cout, k, B, Ho, Wo)
    nbytes = ((splits * ktot * cout * 4 + 7) & ~7) + splits * cout * 8
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x1.device)
    if dw is None:
        dw = torch.empty((ktot, cout), dtype=torch.float32, device=x1.device)
    assert dw.numel() == ktot * cout
    if want_bias and db is None:
        db = torch.empty(cout, dtype=torch.float32, device=x1.device)
    check(lib().cf_conv2d_wgrad(_f32(x1), C1, _opt(x2), C2, _f32(dy), _f32(dw), _opt(db) if want_bias else None, ws.data_ptr(), ws.numel() * 8,
                                B, H, W, cout, k, k, stride, _stream()), "cf_conv2d_wgrad")
    return dw, (db if want_bias else None)


def conv2d_dgrad(dy, wt, in_hw, k, stride=1, ci_off=0, cn=None, dx=None, dx_coff=0, accumulate=False):
    """dX of conv with the weight matrix wt [Cin*k*k, Cout] for the input channels [ci_off, ci_off + cn), written into (accumulate: added
    to) channels [dx_coff, dx_coff + cn) of dx [B, *, H, W]."""
    B, cout = dy.shape[0], dy.shape[1]
    H, W = in_hw
    cin = wt.shape[0] // (k * k)
    assert wt.shape == (cin * k * k, cout), (wt.shape, cin, k, cout)
    assert tuple(dy.shape[2:]) == _out_hw(H, W, k, stride), (dy.shape, in_hw, k, stride)
    cn = cin - ci_off if cn is None else cn
    if dx is None:
        assert not accumulate
        dx = torch.empty((B, dx_coff + cn, H, W), dtype=torch.float32, device=dy.device)
    assert dx.shape[0] == B and tuple(dx.shape[2:]) == (H, W)
    check(lib().cf_conv2d_dgrad(_f32(dy), _f32(wt), _f32(dx), dx.shape[1], dx_coff, ci_off, cn, cin, B, H, W, cout, k, k, stride,
                                1 if accumulate else 0, _stream()), "cf_conv2d_dgrad")
    return dx


def norm_act_bwd(x, dy, ws, gamma, beta, dgamma=None, dbeta=None, eps=EPS, slope=SLOPE):
    """(dx, dgamma, dbeta) of leaky_relu(instance_norm(x) * gamma + beta); ws = ops.group_norm_stats(x, C)."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    assert dy.shape == x.shape and ws.dtype == torch.float64 and ws.numel() >= 2 * B * C
    dx = torch.empty_like(x)
    dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if dgamma is None else dgamma
    dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if dbeta is None else dbeta
    bws = torch.empty(2 * B * C, dtype=torch.float64, device=x.device)
    check(lib().cf_norm_act_bwd(_f32(x), _f32(dy), ws.data_ptr(), _f32(gamma), _f32(beta), _f32(dx), _f32(dgamma), _f32(dbeta), bws.data_ptr(),
                                B, C, HW, float(eps), float(slope), _stream()), "cf_norm_act_bwd")
    return dx, dgamma, dbeta


def dc_ce_loss(logits, target, loss, weight=1.0, want_grad=True, smooth=1e-5, batch_dice=True):
    """One supervised output of MultipleOutputLoss2(DC_and_CE_loss(batch_dice, smooth, do_bg=False)): loss (a device scalar) += weight * l;
    returns (l as a device scalar, weight * dl/dlogits or None).  target: int32 [B, H, W]."""
    if not batch_dice:
        raise ValueError("batch_dice=False is refused: the reference's loss is then a vector of length B and its backward() cannot run")
    B, K = logits.shape[0], logits.shape[1]
    HW = logits.numel() // (B * K)
    if target.dtype != torch.int32 or not target.is_cuda or not target.is_contiguous() or target.numel() != B * HW:
        raise TypeError("target must be a contiguous CUDA int32 tensor of B*H*W labels")
    nb = lib().cf_dc_ce_loss_blocks(B * HW)
    check(min(nb, 0), "cf_dc_ce_loss_blocks")
    part = torch.empty(nb * (1 + 3 * K), dtype=torch.float64, device=logits.device)
    coef = torch.empty(2 * K, dtype=torch.float32, device=logits.device)
    one = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib().cf_dc_ce_loss(_f32(logits), target.data_ptr(), _opt(dl), _f32(loss), _f32(one), _f32(coef), part.data_ptr(), B, K, HW,
                              float(smooth), float(weight), _stream()), "cf_dc_ce_loss")
    return one, dl


def deep_supervision_loss(outputs, targets, weights, want_grad=True, batch_dice=True):
    """MultipleOutputLoss2: sum of weights[i] * DC_and_CE(outputs[i], targets[i]); an output of weight 0 is skipped entirely (its dlogits is
    None).  Returns (loss, a device scalar; [dlogits or None per output])."""
    assert len(outputs) == len(targets) == len(weights)
    loss = torch.zeros(1, dtype=torch.float32, device=outputs[0].device)
    grads = []
    for o, t, w in zip(outputs, targets, weights):
        if w == 0:
            grads.append(None)
            continue
        grads.append(dc_ce_loss(o, t, loss, w, want_grad, batch_dice=batch_dice)[1])
    return loss, grads


# ---- transposed convolution with kernel == stride: a 1x1 convolution to Cout*kh*kw channels, then an interleave ---------------------------
def conv_transpose_fwd(x, w):
    """w in torch's layout [Cin, Cout, kh, kw], kernel == stride in {(2,2), (2,1), (1,2)}, no bias."""
    from . import ops
    cin, cout, kh, kw = w.shape
    if (kh, kw) == (2, 2):
        return ops.conv_transpose2d_k2s2(x, w, None)
    B, _, H, W = x.shape
    y = ops.conv2d(x, w.reshape(cin, cout * kh * kw), None, cout * kh * kw, 1, 1)
    return y.view(B, cout, kh, kw, H, W).permute(0, 1, 4, 2, 5, 3).reshape(B, cout, H * kh, W * kw)


def conv_transpose_bwd(x, w, dy, dw=None, dx=None, accumulate=False):
    """(dx, dw in torch's layout): dy is de-interleaved (a view and a copy), then the 1x1 dgrad and wgrad run.  dx / accumulate as in
    conv2d_dgrad; dw: a destination of w's shape."""
    cin, cout, kh, kw = w.shape
    B, _, H, W = x.shape
    d = dy.view(B, cout, H, kh, W, kw).permute(0, 1, 3, 5, 2, 4).reshape(B, cout * kh * kw, H, W).contiguous()
    dx = conv2d_dgrad(d, w.view(cin, cout * kh * kw), (H, W), 1, dx=dx, accumulate=accumulate)
    dw, _ = conv2d_wgrad(x, d, 1, dw=None if dw is None else dw.view(cin, cout * kh * kw))
    return dx, dw.view(cin, cout, kh, kw)


# ---- 3x3 convolution with a per-axis stride (the plans' (2,1) stage): stride 1, then subsampling, as inference runs it ---------------------
def subsample(y, stride):
    return y[:, :, ::stride[0], ::stride[1]].contiguous()


def scatter_stride(dy, full_hw, stride):
    """the adjoint of subsample: dy placed on the stride grid of a zero map"""
    z = torch.zeros(dy.shape[:2] + tuple(full_hw), dtype=dy.dtype, device=dy.device)
    z[:, :, ::stride[0], ::stride[1]] = dy
    return z


# ---- optimizer ------------------------------------------------------------------------------------------------------------------------
def grad_norm(grad, table, ntensors, max_norm=12.0):
    """-> device [2]: torch's total_norm over the tensors with a gradient, and the clip factor min(1, max_norm / (norm + 1e-6))"""
    tn = torch.empty(ntensors, dtype=torch.float32, device=grad.device)
    out = torch.empty(2, dtype=torch.float32, device=grad.device)
    assert table.dtype == torch.int64 and table.is_cuda and table.numel() == 3 * ntensors
    check(lib().cf_grad_norm(_f32(grad), table.data_ptr(), ntensors, float(max_norm), _f32(tn), _f32(out), _stream()), "cf_grad_norm")
    return out


def sgd_nesterov(param, grad, mom, table, ntensors, max_size, clip, lr, weight_decay=3e-5, momentum=0.99, first=False):
    assert param.numel() == grad.numel() == mom.numel() and table.dtype == torch.int64 and table.is_cuda
    check(lib().cf_sgd_nesterov(_f32(param), _f32(grad), _f32(mom), table.data_ptr(), ntensors, int(max_size), _f32(clip), float(lr),
                                float(weight_decay), float(momentum), 1 if first else 0, _stream()), "cf_sgd_nesterov")
