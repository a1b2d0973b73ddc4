"""The training kernels (csrc/conv_grad.hip, csrc/train_ops.hip) one by one, held to fp64 torch autograd on the CPU by the yardstick of
tests/_train_refs.py: the device error may be at most 4 x the error of the same computation in fp32 torch on the CPU (floor 1e-6), by
|g - g64| / max(|g64|, 1e-3 |all gradients of the call|).  Every call is repeated and must give the same bits.

  cf_conv2d_wgrad / cf_conv2d_dgrad   Cin in {1, 5, 16} x Cout in {3, 8, 40} (tails of every 32-wide tile) on 7x9 (less than one tile, odd),
                                      40x48 and 9x9 at stride 2 (odd, Ho = 5), 3x3 and 1x1, B in {1, 3}; cat[5 + 8]; dgrad into a channel
                                      sub-range with accumulate off and on; one shape with exactly one K split and one with several;
                                      transposed convolutions (2,2), (2,1), (1,2); the per-axis-stride route
  cf_norm_act_bwd                     planes of 2x3 (a bottleneck) and 40x48, C = 8, B = 2
  cf_dc_ce_loss                       K = 4 and 2, B = 2, 8x12; a class absent from the batch; a zero-weight output; batch_dice=False refused
  cf_grad_norm / cf_sgd_nesterov      three steps against clip_grad_norm_ + torch.optim.SGD(nesterov, weight decay) in fp32 on the CPU, norm
                                      above and below 12, within 2 ulp per element (above 12 in two parts, see the test's docstring); a
                                      masked tensor unchanged bit for bit"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _train_refs as R

pytestmark = pytest.mark.gpu


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def _conv_truth(x, w, b, dy, stride, pad, dtype):
    x_, w_, b_ = (R.leaf(t, dtype) for t in (x, w, b))
    y = F.conv2d(x_, w_, b_, stride=stride, padding=pad)
    y.backward(dy.to(dtype))
    return x_.grad, w_.grad, b_.grad


def _check_conv(dev, gen, B, C1, C2, H, W, cout, k, stride, label):
    from cineflow import ops, train_ops as T
    cin = C1 + C2
    x, w, b = _rand(gen, B, cin, H, W), _rand(gen, cout, cin, k, k) / np.sqrt(cin * k * k), _rand(gen, cout)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    dy = _rand(gen, B, cout, Ho, Wo)
    dx64, dw64, db64 = _conv_truth(x, w, b, dy, stride, k // 2, torch.float64)
    dx32, dw32, db32 = _conv_truth(x, w, b, dy, stride, k // 2, torch.float32)
    x1 = x[:, :C1].float().contiguous().to(dev)
    x2 = x[:, C1:].float().contiguous().to(dev) if C2 else None
    dyd = dy.float().to(dev)
    wm = ops.prep_conv_weight(w.float()).to(dev)
    dw, db = T.conv2d_wgrad(x1, dyd, k, stride=stride, x2=x2, want_bias=True)
    dx = T.conv2d_dgrad(dyd, wm, (H, W), k, stride=stride)
    dw2, db2 = T.conv2d_wgrad(x1, dyd, k, stride=stride, x2=x2, want_bias=True)
    dx2 = T.conv2d_dgrad(dyd, wm, (H, W), k, stride=stride)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dx, dx2), "%s: a repeated call changed bits" % label
    alln = R.total_norm([dx64, dw64, db64])
    dw_ref_layout = dw.cpu().t().reshape(cout, cin, k, k)
    R.hold(label + " dW", dw_ref_layout, dw32, dw64, alln)
    R.hold(label + " db", db, db32, db64, alln)
    R.hold(label + " dX", dx, dx32, dx64, alln)
    return dx, dx64, dx32, alln, (dyd, wm)


MAPS = [(7, 9, 1), (40, 48, 1), (9, 9, 2)]


@pytest.mark.parametrize("H,W,stride", MAPS)
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_wgrad_dgrad(dev, H, W, stride, k, B):
    gen = torch.Generator().manual_seed(1000 * H + 10 * k + B)
    for cin, cout in itertools.product((1, 5, 16), (3, 8, 40)):
        _check_conv(dev, gen, B, cin, 0, H, W, cout, k, stride, "B%d %dx%d s%d k%d %d->%d" % (B, H, W, stride, k, cin, cout))


def test_wgrad_dgrad_cat_and_channel_ranges(dev):
    """cat[5 + 8]: both inputs feed dW; dX goes to each part's own tensor, into a channel sub-range, overwriting and accumulating"""
    from cineflow import train_ops as T
    gen = torch.Generator().manual_seed(7)
    B, H, W = 2, 11, 13
    dx, dx64, dx32, alln, (dyd, wm) = _check_conv(dev, gen, B, 5, 8, H, W, 8, 3, 1, "cat 5+8")
    sentinel = 1234.5
    wide = torch.full((B, 12, H, W), sentinel, device=dev)
    T.conv2d_dgrad(dyd, wm, (H, W), 3, ci_off=5, cn=8, dx=wide, dx_coff=2)
    assert torch.equal(wide[:, 2:10], dx[:, 5:13]) and bool((wide[:, :2] == sentinel).all()) and bool((wide[:, 10:] == sentinel).all())
    first = torch.full((B, 12, H, W), sentinel, device=dev)
    first[:, 2:10] = torch.randn(B, 8, H, W, generator=gen).to(dev)
    base = first.clone()
    T.conv2d_dgrad(dyd, wm, (H, W), 3, ci_off=5, cn=8, dx=first, dx_coff=2, accumulate=True)
    assert torch.equal(first[:, 2:10], base[:, 2:10] + dx[:, 5:13]), "accumulate is one rounded add on what the destination held"
    assert bool((first[:, :2] == sentinel).all()) and bool((first[:, 10:] == sentinel).all())
    part = T.conv2d_dgrad(dyd, wm, (H, W), 3, ci_off=0, cn=5)
    assert torch.equal(part, dx[:, :5])


def test_wgrad_one_split_and_several(dev):
    from cineflow import train_ops as T
    gen = torch.Generator().manual_seed(11)
    assert T.wgrad_splits(16, 8, 3, 1, 7, 9) == 1
    _check_conv(dev, gen, 1, 16, 0, 7, 9, 8, 3, 1, "one split")
    n = T.wgrad_splits(16, 8, 3, 3, 40, 48)
    assert n > 1
    # a pixel count that is odd and no multiple of the chunk: the last split is short, the last pixel pair half empty
    assert T.wgrad_splits(4, 8, 3, 3, 21, 29) > 1
    _check_conv(dev, gen, 3, 4, 0, 21, 29, 8, 3, 1, "several splits, odd pixel count")


@pytest.mark.parametrize("kernel", [(2, 2), (2, 1), (1, 2)])
def test_transposed_convolution_route(dev, kernel):
    from cineflow import train_ops as T
    gen = torch.Generator().manual_seed(5 + kernel[0] * 3 + kernel[1])
    B, cin, cout, H, W = 2, 12, 5, 5, 7
    x, w = _rand(gen, B, cin, H, W), _rand(gen, cin, cout, *kernel) / np.sqrt(cin)
    dy = _rand(gen, B, cout, H * kernel[0], W * kernel[1])
    res = {}
    for dt in (torch.float64, torch.float32):
        x_, w_ = R.leaf(x, dt), R.leaf(w, dt)
        y = F.conv_transpose2d(x_, w_, stride=kernel)
        y.backward(dy.to(dt))
        res[dt] = (y.detach(), x_.grad, w_.grad)
    xd, wd, dyd = x.float().to(dev), w.float().to(dev), dy.float().to(dev)
    y = T.conv_transpose_fwd(xd, wd)
    dx, dw = T.conv_transpose_bwd(xd, wd, dyd)
    dx2, dw2 = T.conv_transpose_bwd(xd, wd, dyd)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    alln = R.total_norm(res[torch.float64][1:])
    R.hold("convT %s y" % (kernel,), y, res[torch.float32][0], res[torch.float64][0], R.total_norm([res[torch.float64][0]]))
    R.hold("convT %s dX" % (kernel,), dx, res[torch.float32][1], res[torch.float64][1], alln)
    R.hold("convT %s dW" % (kernel,), dw, res[torch.float32][2], res[torch.float64][2], alln)


@pytest.mark.parametrize("stride", [(2, 1), (1, 2)])
def test_per_axis_stride_route(dev, stride):
    """a 3x3 convolution with stride (2,1): stride 1 plus subsampling forward, dY scattered into zeros and the stride-1 kernels backward"""
    from cineflow import ops, train_ops as T
    gen = torch.Generator().manual_seed(21 + stride[0])
    B, cin, cout, H, W = 2, 6, 9, 10, 7
    x, w, b = _rand(gen, B, cin, H, W), _rand(gen, cout, cin, 3, 3) / np.sqrt(9 * cin), _rand(gen, cout)
    Ho, Wo = (H - 1) // stride[0] + 1, (W - 1) // stride[1] + 1
    dy = _rand(gen, B, cout, Ho, Wo)
    d64, d32 = (_conv_truth(x, w, b, dy, stride, 1, dt) for dt in (torch.float64, torch.float32))
    xd, wm, bd = x.float().to(dev), ops.prep_conv_weight(w.float()).to(dev), b.float().to(dev)
    y = T.subsample(ops.conv2d(xd, wm, bd, cout, 3, 3, stride=1, pad=(1, 1)), stride)
    y64 = F.conv2d(x, w, b, stride=stride, padding=1)
    assert y.shape == y64.shape and float((y.cpu().double() - y64).abs().max()) <= 2e-5
    full = T.scatter_stride(dy.float().to(dev), (H, W), stride)
    dw, db = T.conv2d_wgrad(xd, full, 3, want_bias=True)
    dx = T.conv2d_dgrad(full, wm, (H, W), 3)
    alln = R.total_norm(d64)
    R.hold("stride %s dX" % (stride,), dx, d32[0], d64[0], alln)
    R.hold("stride %s dW" % (stride,), dw.cpu().t().reshape(cout, cin, 3, 3), d32[1], d64[1], alln)
    R.hold("stride %s db" % (stride,), db, d32[2], d64[2], alln)


@pytest.mark.parametrize("H,W", [(2, 3), (40, 48)])
def test_norm_act_bwd(dev, H, W):
    from cineflow import ops, train_ops as T
    gen = torch.Generator().manual_seed(H)
    B, C = 2, 8
    x, dy = _rand(gen, B, C, H, W) * 2 + 0.5, _rand(gen, B, C, H, W)
    gamma, beta = 1 + 0.3 * _rand(gen, C), 0.2 * _rand(gen, C)
    res = {}
    for dt in (torch.float64, torch.float32):
        x_, g_, b_ = (R.leaf(t, dt) for t in (x, gamma, beta))
        y = F.leaky_relu(F.instance_norm(x_, weight=g_, bias=b_, eps=1e-5), 0.01)
        y.backward(dy.to(dt))
        res[dt] = (x_.grad, g_.grad, b_.grad)
    xd, dyd, gd, bd = (t.float().to(dev) for t in (x, dy, gamma, beta))
    ws = ops.group_norm_stats(xd, C)
    out = T.norm_act_bwd(xd, dyd, ws, gd, bd)
    out2 = T.norm_act_bwd(xd, dyd, ws, gd, bd)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    alln = R.total_norm(res[torch.float64])
    for nm, o, a32, a64 in zip(("dx", "dgamma", "dbeta"), out, res[torch.float32], res[torch.float64]):
        R.hold("norm bwd %dx%d %s" % (H, W, nm), o, a32, a64, alln)


def _loss_inputs(K, absent=None, seed=3):
    gen = torch.Generator().manual_seed(seed + K)
    B, H, W = 2, 8, 12
    logits = [_rand(gen, B, K, H, W) * 2, _rand(gen, B, K, H // 2, W // 2) * 2, _rand(gen, B, K, H // 4, W // 4)]
    targets = [torch.randint(0, K, l.shape[:1] + l.shape[2:], generator=gen) for l in logits]
    if absent is not None:
        targets = [torch.where(t == absent, torch.zeros_like(t), t) for t in targets]
    return logits, targets


@pytest.mark.parametrize("K,absent", [(4, None), (2, None), (4, 2)])
def test_dc_ce_loss(dev, K, absent):
    from cineflow import train_ops as T
    logits, targets = _loss_inputs(K, absent)
    weights = [2 / 3, 1 / 3, 0.0]
    res = {}
    for dt in (torch.float64, torch.float32):
        ls = [R.leaf(l, dt) for l in logits]
        loss = R.multiple_output_loss(ls, targets, weights)
        loss.backward()
        res[dt] = (loss.detach(), [l.grad for l in ls])
    assert res[torch.float64][1][2] is None
    ld = [l.float().to(dev) for l in logits]
    td = [t.to(torch.int32).to(dev) for t in targets]
    loss, grads = T.deep_supervision_loss(ld, td, weights)
    loss2, grads2 = T.deep_supervision_loss(ld, td, weights)
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads[:2], grads2[:2]))
    assert grads[2] is None, "a zero-weight output is skipped entirely: no dlogits is written"
    R.hold_scalar("loss K=%d absent=%s" % (K, absent), loss.item(), res[torch.float32][0], res[torch.float64][0])
    alln = R.total_norm(res[torch.float64][1][:2])
    for i in range(2):
        R.hold("dlogits[%d] K=%d absent=%s" % (i, K, absent), grads[i], res[torch.float32][1][i], res[torch.float64][1][i], alln)


def test_dc_ce_loss_matches_the_reference_fixture(dev, golden):
    """the outputs of the reference's own MultipleOutputLoss2(DC_and_CE_loss) on committed inputs (tests/golden/make_golden_train.py)"""
    from cineflow import train_ops as T
    g = golden("train/loss")
    n = int(g["n_outputs"])
    weights = [float(v) for v in g["weights"]]
    ld = [torch.from_numpy(g["logits%d" % i]).float().to(dev) for i in range(n)]
    td = [torch.from_numpy(g["target%d" % i]).to(torch.int32).to(dev) for i in range(n)]
    loss, grads = T.deep_supervision_loss(ld, td, weights)
    R.hold_scalar("loss vs reference fixture", loss.item(), g["loss32"], g["loss64"])
    alln = R.total_norm([torch.from_numpy(g["grad64_%d" % i]) for i in range(n) if weights[i] != 0])
    for i in range(n):
        if weights[i] == 0:
            assert grads[i] is None
            continue
        R.hold("dlogits[%d] vs reference fixture" % i, grads[i], torch.from_numpy(g["grad32_%d" % i]), torch.from_numpy(g["grad64_%d" % i]), alln)


def test_batch_dice_false_is_refused(dev):
    from cineflow import train_ops as T
    logits, targets = _loss_inputs(4)
    with pytest.raises(ValueError, match="batch_dice"):
        T.deep_supervision_loss([logits[0].float().to(dev)], [targets[0].to(torch.int32).to(dev)], [1.0], batch_dice=False)


def _ulp_distance(a, b):
    ia, ib = (t.contiguous().view(torch.int32).to(torch.int64) for t in (a, b))
    ia, ib = (torch.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("scale,clipped", [(1.0, True), (1e-3, False)])
def test_clip_and_nesterov_sgd(dev, scale, clipped):
    """Three steps of clip_grad_norm_(12) + torch.optim.SGD(nesterov, weight decay) in fp32 on the CPU, element by element within 2 ulp.
    Below the clipping norm the factor is exactly 1 on both sides and the whole pipeline is compared as it stands (measured: every element
    equal).  Above it, torch's own fp32 total_norm carries summation error: measured on these tensors 78.7296982 against the correctly
    rounded 78.7296906 the device gives from its fp64 sums, one ulp apart -- the clip factors then differ in the last bit, every gradient
    by up to an ulp OF THE GRADIENT, and parameters near zero by hundreds of ulp of themselves (1014 of 5760 elements, up to 384 ulp).  No
    summation order on the device can reproduce another machine's vectorised fp32 sum, so the check is taken in two parts that together
    ask the same: the device's norm agrees with clip_grad_norm_'s to 4 fp32 ulp (both are roundings of one number; torch's sum over 5760
    squares is itself good to a few ulp), and the element chain is held to 2 ulp against torch's SGD fed the gradients scaled the way
    clip_grad_norm_ scales them (g.mul_(factor)) with the factor under test."""
    from cineflow import train_ops as T
    gen = torch.Generator().manual_seed(9)
    shapes = [(40, 16, 3, 3), (40,), (7,), (16, 8, 2, 2), (1, 5)]
    masked = 2
    params = [torch.nn.Parameter(torch.randn(s, generator=gen) * 0.1) for s in shapes]
    init = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    sizes = [int(np.prod(s)) for s in shapes]
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 3) & ~3
    table = torch.tensor([[offs[i], sizes[i], 0 if i == masked else 1] for i in range(len(shapes))], dtype=torch.int64).to(dev)
    P = torch.zeros(o, device=dev)
    for i, p in enumerate(init):
        P[offs[i]:offs[i] + sizes[i]] = p.flatten().to(dev)
    M = torch.full((o,), 77.0, device=dev)                     # the first step must not read it
    lrs = [1e-2, 9e-3, 8e-3]
    for step in range(3):
        grads = [torch.randn(s, generator=gen) * scale for s in shapes]
        G = torch.zeros(o, device=dev)
        for i, g in enumerate(grads):
            G[offs[i]:offs[i] + sizes[i]] = g.flatten().to(dev)
        nc = T.grad_norm(G, table, len(shapes), 12.0).cpu()
        for i, p in enumerate(params):
            p.grad = None if i == masked else grads[i].clone()
        if clipped:                  # torch's norm alone, on throw-away copies; the real gradients are scaled below
            shadow = [torch.nn.Parameter(p.detach().clone()) for p in params]
            for sp, p in zip(shadow, params):
                sp.grad = None if p.grad is None else p.grad.clone()
            total = torch.nn.utils.clip_grad_norm_(shadow, 12)
        else:
            total = torch.nn.utils.clip_grad_norm_(params, 12)
        print("step %d: total norm torch %.9g device %.9g; clip %.9g" % (step, float(total), float(nc[0]), float(nc[1])))
        assert (float(total) > 12) == clipped
        assert abs(float(nc[0]) - float(total)) <= 4 * 2.0 ** -23 * float(total)
        assert (float(nc[1]) < 1.0) == clipped
        if clipped:
            assert nc[1] == torch.clamp(12.0 / (nc[0] + 1e-6), max=1.0), "the factor is clip_grad_norm_'s own fp32 expression of the device's norm"
            for i, p in enumerate(params):
                if i != masked:
                    p.grad.mul_(nc[1])
        for gr in opt.param_groups:
            gr["lr"] = lrs[step]
        opt.step()
        T.sgd_nesterov(P, G, M, table, len(shapes), max(sizes), nc.to(dev), lrs[step], 3e-5, 0.99, first=step == 0)
    for i, p in enumerate(params):
        got = P[offs[i]:offs[i] + sizes[i]].cpu()
        if i == masked:
            assert torch.equal(got, init[i].flatten()), "a tensor without a gradient is untouched: no weight decay either"
            assert bool((M[offs[i]:offs[i] + sizes[i]] == 77.0).all())
            continue
        d = _ulp_distance(got, p.detach().flatten())
        print("tensor %d: max ulp distance after three steps %d, %d of %d elements differ" % (i, d, int((got != p.detach().flatten()).sum()), sizes[i]))
        assert d <= 2, (i, d)
