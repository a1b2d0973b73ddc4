"""cf_tta_accumulate_nonlin, cf_tta_accumulate_3d_nonlin and cf_region_labels (region-based heads: one sigmoid channel per region, labels
painted in regions_class_order) against fp64 / numpy references.

Bars.  The sigmoid accumulate is held to 1e-6 against the fp64 sigmoid: outputs lie in [0, 1] and 1e-6 is the bar of the softmax twin
(tests/test_gpu_ops.py::test_tta_and_tiles).  nonlin = softmax launches the kernel of cf_tta_accumulate[_3d] itself: bit-identical.  The 3-D
entry at D = 1 runs the kernel of the 2-D entry: bit-identical.  cf_region_labels is integer logic on fp32 comparisons: equal to the numpy loop.

entry point -> kernel -> test
  cf_tta_accumulate_nonlin     tta_accumulate_sigmoid_kernel<4> (W % 4 == 0, no flip_w) / <1>     test_sigmoid_2d_flips, test_second_trips, ...
  cf_tta_accumulate_3d_nonlin  the same two kernels with D > 1                                       test_sigmoid_3d_flips, test_3d_depth_one_is_the_2d_kernel
  cf_region_labels             region_labels_kernel<4> (HW % 4 == 0) / <1>                           test_region_labels

Measured on the MI355X (pytest -s prints each figure): the sigmoid accumulate against fp64 at most 1.4e-7 on the small 2-D rows, 1.8e-7
with eight 3-D flips at 1/8, 2.8e-7 on the two second-trip rows (accumulators of unit scale); every bit-identity and label row exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 1e-6
TRIP1 = 4096 * 256            # common.h flat_grid: at most 4096 blocks of 256 threads per trip
SOFTMAX, SIGMOID = 0, 1


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def sigmoid64(t):
    return 1.0 / (1.0 + torch.exp(-t.double()))


def worst(name, got, ref):
    d = float((got.double().cpu() - ref.double()).abs().max())
    print("  %-64s max |diff| %.3e (bar %.0e)" % (name, d, BAR))
    return d


def raw(name, *args):
    from cineflow import _lib
    return getattr(_lib.lib(), name)(*args), _lib.lib().cf_last_error().decode()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def flipped(t, dims):
    return torch.flip(t, dims).contiguous() if dims else t.contiguous()


@pytest.mark.parametrize("shape", [(2, 3, 7, 5), (2, 3, 6, 8), (2, 1, 7, 5), (1, 1, 5, 12)])
def test_sigmoid_2d_flips(dev, shape):
    """each flip alone into a zero buffer, then the four at weight 1/4; W = 5 takes the scalar kernel, W = 8 / 12 the 16-byte one for
    the flips without flip_w; K = 1 included.  Measured: <= 1.3e-7 in every row."""
    from cineflow import ops
    print()
    B, K, H, W = shape
    logits = 3 * randn(B, K, H, W, seed=401 + W)
    ref = sigmoid64(logits)
    acc4 = torch.zeros(B, K, H, W, device=dev)
    for fh, fw in ((0, 0), (0, 1), (1, 0), (1, 1)):
        dims = tuple(d for d, f in ((2, fh), (3, fw)) if f)
        lin = flipped(logits, dims).to(dev)
        acc = torch.zeros(B, K, H, W, device=dev)
        ops.tta_accumulate(lin, acc, fh, fw, 1.0, nonlin="sigmoid")
        assert worst("%s flip (%d, %d) alone" % (shape, fh, fw), acc, ref) <= BAR
        assert float(acc.min()) >= 0.0 and float(acc.max()) <= 1.0
        ops.tta_accumulate(lin, acc4, fh, fw, 0.25, nonlin="sigmoid")
    assert worst("%s four flips at 1/4" % (shape,), acc4, ref) <= BAR


def test_sigmoid_accumulates_onto_what_is_there(dev):
    from cineflow import ops
    print()
    logits, acc0 = randn(2, 3, 6, 8, seed=411), randn(2, 3, 6, 8, seed=412)
    for fw in (0, 1):
        acc = acc0.clone().to(dev)
        ops.tta_accumulate(flipped(logits, (3,) if fw else ()).to(dev), acc, 0, fw, 0.7, nonlin="sigmoid")
        assert worst("acc0 + 0.7 sigmoid, flip_w %d" % fw, acc, acc0.double() + 0.7 * sigmoid64(logits)) <= BAR


@pytest.mark.parametrize("W", [8, 7])
def test_saturated_logits_give_exact_zero_and_one(dev, W):
    from cineflow import ops
    vals = torch.tensor([100.0, -100.0, 30.0, -30.0, 0.0, 88.0, -88.0, 89.0, -89.0, 1e30, -1e30, float("inf"), float("-inf")])
    logits = vals.repeat(2 * 2 * 3 * W)[:2 * 2 * 3 * W].reshape(2, 2, 3, W).contiguous()
    acc = torch.zeros(2, 2, 3, W, device=dev)
    ops.tta_accumulate(logits.to(dev), acc, 0, 0, 1.0, nonlin="sigmoid")
    got = acc.cpu()
    assert not bool(torch.isnan(got).any())
    assert bool((got[logits >= 89.0] == 1.0).all()) and bool((got[logits <= -89.0] == 0.0).all())
    assert bool((got[logits == 100.0] == 1.0).all()) and bool((got[logits == -100.0] == 0.0).all())
    assert float((got.double() - sigmoid64(logits)).abs().max()) <= BAR              # +-30, +-88 and 0 within the bar
    assert bool((got[logits == 0.0] == 0.5).all())


@pytest.mark.parametrize("W", [8, 7])
def test_channels_are_independent(dev, W):
    """changing channel j's logits leaves channel i's output bit-identical (a softmax fails this)"""
    from cineflow import ops
    a = randn(2, 3, 5, W, seed=421)
    b = a.clone()
    b[:, 1] = 5 * randn(2, 5, W, seed=422)
    outs = {}
    for nonlin in ("sigmoid", "softmax"):
        for name, t in (("a", a), ("b", b)):
            acc = torch.zeros(2, 3, 5, W, device=dev)
            ops.tta_accumulate(t.to(dev), acc, 0, 0, 1.0, nonlin=nonlin)
            outs[nonlin, name] = acc.cpu()
    for i in (0, 2):
        assert torch.equal(outs["sigmoid", "a"][:, i], outs["sigmoid", "b"][:, i])
        assert not torch.equal(outs["softmax", "a"][:, i], outs["softmax", "b"][:, i])
    assert not torch.equal(outs["sigmoid", "a"][:, 1], outs["sigmoid", "b"][:, 1])


def test_softmax_form_is_the_existing_kernel(dev):
    logits, acc0 = 2 * randn(2, 4, 9, 10, seed=431), randn(2, 4, 9, 10, seed=432)
    x = logits.to(dev)
    for fh, fw in ((0, 0), (1, 1)):
        a, b = acc0.clone().to(dev), acc0.clone().to(dev)
        assert raw("cf_tta_accumulate", ptr(x), ptr(a), 2, 4, 9, 10, fh, fw, 0.25, None)[0] == 0
        assert raw("cf_tta_accumulate_nonlin", ptr(x), ptr(b), 2, 4, 9, 10, fh, fw, 0.25, SOFTMAX, None)[0] == 0
        assert torch.equal(a, b)
    x3 = 2 * randn(1, 3, 3, 6, 5, seed=433)
    a, b = torch.zeros(1, 3, 3, 6, 5, device=dev), torch.zeros(1, 3, 3, 6, 5, device=dev)
    assert raw("cf_tta_accumulate_3d", ptr(x3.to(dev)), ptr(a), 1, 3, 3, 6, 5, 1, 0, 1, 0.125, None)[0] == 0
    assert raw("cf_tta_accumulate_3d_nonlin", ptr(x3.to(dev)), ptr(b), 1, 3, 3, 6, 5, 1, 0, 1, 0.125, SOFTMAX, None)[0] == 0
    assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_second_trips(dev):
    """more work items than one trip of the grid holds, both access forms; both flips that the form allows.  Measured: 2.8e-7 both."""
    from cineflow import ops
    print()
    for (B, K, H, W), (fh, fw) in (((1, 3, 600, 601), (1, 1)), ((1, 3, 1200, 1180), (1, 0))):
        n = B * K * H * W
        assert (n if W % 4 else n // 4) > TRIP1
        logits, acc0 = 2 * randn(B, K, H, W, seed=441), randn(B, K, H, W, seed=442)
        acc = acc0.clone().to(dev)
        dims = tuple(d for d, f in ((2, fh), (3, fw)) if f)
        ops.tta_accumulate(flipped(logits, dims).to(dev), acc, fh, fw, 0.7, nonlin="sigmoid")
        ref = acc0.double() + 0.7 * sigmoid64(logits)
        assert worst("%d x %d x %d x %d, flips (%d, %d)" % (B, K, H, W, fh, fw), acc, ref) <= BAR
        tail = (acc.cpu().double() - ref).flatten()[(TRIP1 * (1 if W % 4 else 4)):]
        assert tail.numel() > 0 and float(tail.abs().max()) <= BAR


@pytest.mark.parametrize("shape", [(3, 6, 5), (2, 3, 8)])
def test_sigmoid_3d_flips(dev, shape):
    """the eight flips alone, then all at 1/8; (3, 6, 5) is the scalar kernel, (2, 3, 8) the 16-byte one where flip_w is off"""
    from cineflow import ops
    print()
    D, H, W = shape
    logits = 3 * randn(2, 3, D, H, W, seed=451)
    ref = sigmoid64(logits)
    acc8 = torch.zeros(2, 3, D, H, W, device=dev)
    for m in range(8):
        f = (m >> 2 & 1, m >> 1 & 1, m & 1)
        dims = tuple(d for d, on in zip((2, 3, 4), f) if on)
        lin = flipped(logits, dims).to(dev)
        acc = torch.zeros(2, 3, D, H, W, device=dev)
        ops.tta_accumulate_3d(lin, acc, f[0], f[1], f[2], 1.0, nonlin="sigmoid")
        assert worst("%s flip %s alone" % (shape, f), acc, ref) <= BAR
        ops.tta_accumulate_3d(lin, acc8, f[0], f[1], f[2], 0.125, nonlin="sigmoid")
    assert worst("%s eight flips at 1/8" % (shape,), acc8, ref) <= BAR


@pytest.mark.parametrize("W", [8, 5])
def test_3d_depth_one_is_the_2d_kernel(dev, W):
    from cineflow import ops
    logits, acc0 = 2 * randn(2, 3, 6, W, seed=461), randn(2, 3, 6, W, seed=462)
    for fh, fw in ((0, 0), (1, 0), (0, 1), (1, 1)):
        a, b = acc0.clone().to(dev), acc0.clone().to(dev)[:, :, None].contiguous()
        ops.tta_accumulate(logits.to(dev), a, fh, fw, 0.3, nonlin="sigmoid")
        ops.tta_accumulate_3d(logits.to(dev)[:, :, None].contiguous(), b, 0, fh, fw, 0.3, nonlin="sigmoid")
        assert torch.equal(a, b[:, :, 0])


def numpy_region_labels(probs, order):
    seg = np.zeros((probs.shape[0],) + probs.shape[2:], dtype=np.uint8)
    for b in range(probs.shape[0]):
        for i, c in enumerate(order):
            seg[b][probs[b, i] > 0.5] = c
    return seg


@pytest.mark.parametrize("K,HW,order", [(3, 37, (1, 2, 3)), (3, 37, (2, 1, 3)), (2, 37, (1, 2)), (3, 40, (1, 2, 3)), (3, 40, (7, 0, 255))])
def test_region_labels(dev, K, HW, order):
    """B = 2; HW = 37 is the one-voxel kernel, HW = 40 the four-voxel one.  The first voxels hold the threshold cases: exactly 0.5 (not
    taken), nextafter(0.5, 1) (taken), no region set (0), a later region overwriting an earlier one, an earlier one standing alone."""
    from cineflow import ops
    probs = torch.rand(2, K, HW, generator=torch.Generator().manual_seed(471 + HW)).numpy()
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    probs[:, :, 0] = 0.5                                   # nothing taken -> 0
    probs[:, :, 1] = 0.5
    probs[:, 0, 1] = up                                    # region 0 alone, by one ulp
    probs[:, :, 2] = 0.1                                   # no region set -> 0
    probs[:, :, 3] = 0.9                                   # all set: the last one's label
    probs[:, :, 4] = 0.9
    probs[:, K - 1, 4] = 0.5                               # the last one exactly at the threshold: the one before it stays
    ref = numpy_region_labels(probs, order)
    assert (ref[:, 0] == 0).all() and (ref[:, 1] == order[0]).all() and (ref[:, 2] == 0).all() and (ref[:, 3] == order[K - 1]).all()
    assert (ref[:, 4] == order[K - 2]).all()
    got = ops.region_labels(torch.from_numpy(probs).to(dev), order)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, HW)
    assert np.array_equal(got.cpu().numpy(), ref)
    vol = torch.from_numpy(probs[:, :, :36].reshape(2, K, 3, 4, 3).copy()).to(dev)          # trailing dimensions are kept
    assert np.array_equal(ops.region_labels(vol, order).cpu().numpy(), ref[:, :36].reshape(2, 3, 4, 3))


def test_region_labels_second_trip(dev):
    from cineflow import ops
    for HW in (TRIP1 * 4 + 4 * 77, TRIP1 + 77):
        probs = torch.rand(1, 2, HW, generator=torch.Generator().manual_seed(481))
        got = ops.region_labels(probs.to(dev), (1, 2)).cpu().numpy()
        assert np.array_equal(got, numpy_region_labels(probs.numpy(), (1, 2)))


def test_argument_errors(dev):
    from cineflow import ops
    x, acc = torch.zeros(1, 2, 4, 4, device=dev), torch.zeros(1, 2, 4, 4, device=dev)
    seg = torch.zeros(1, 16, dtype=torch.uint8, device=dev)
    order = (ctypes.c_uint8 * 2)(1, 2)
    po = ctypes.cast(order, ctypes.c_void_p)
    for nonlin in (2, -1):
        rc, msg = raw("cf_tta_accumulate_nonlin", ptr(x), ptr(acc), 1, 2, 4, 4, 0, 0, 1.0, nonlin, None)
        assert rc == -1 and "nonlin" in msg
        rc, msg = raw("cf_tta_accumulate_3d_nonlin", ptr(x), ptr(acc), 1, 2, 1, 4, 4, 0, 0, 0, 1.0, nonlin, None)
        assert rc == -1 and "nonlin" in msg
    for nonlin in (SOFTMAX, SIGMOID):
        assert raw("cf_tta_accumulate_nonlin", None, ptr(acc), 1, 2, 4, 4, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_nonlin", ptr(x), None, 1, 2, 4, 4, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_nonlin", ptr(x), ptr(acc), 1, 0, 4, 4, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_nonlin", ptr(x), ptr(acc), 1, 2, 4, 0, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_3d_nonlin", None, ptr(acc), 1, 2, 1, 4, 4, 0, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_3d_nonlin", ptr(x), ptr(acc), 1, 2, 0, 4, 4, 0, 0, 0, 1.0, nonlin, None)[0] == -1
        assert raw("cf_tta_accumulate_3d_nonlin", ptr(x), ptr(acc), 0, 2, 1, 4, 4, 0, 0, 0, 1.0, nonlin, None)[0] == -1
    assert float(acc.abs().max()) == 0.0                                        # nothing was launched
    assert raw("cf_region_labels", None, ptr(seg), 1, 2, 16, po, None)[0] == -1
    assert raw("cf_region_labels", ptr(x), None, 1, 2, 16, po, None)[0] == -1
    assert raw("cf_region_labels", ptr(x), ptr(seg), 1, 2, 16, None, None)[0] == -1
    rc, msg = raw("cf_region_labels", ptr(x), ptr(seg), 1, 0, 16, po, None)
    assert rc == -1 and "K = 0" in msg
    rc, msg = raw("cf_region_labels", ptr(x), ptr(seg), 1, 256, 16, po, None)
    assert rc == -1 and "K = 256" in msg
    assert raw("cf_region_labels", ptr(x), ptr(seg), 1, 2, 0, po, None)[0] == -1
    assert raw("cf_region_labels", ptr(x), ptr(seg), 1, 2, -3, po, None)[0] == -1
    with pytest.raises(ValueError, match="nonlin"):
        ops.tta_accumulate(x, acc, 0, 0, 1.0, nonlin="tanh")
    with pytest.raises(ValueError, match="nonlin"):
        ops.tta_accumulate_3d(x[:, :, None].contiguous(), acc[:, :, None].contiguous(), 0, 0, 0, 1.0, nonlin="tanh")
    with pytest.raises(ValueError, match="one label in 0..255 per region channel"):
        ops.region_labels(x, (1, 2, 3))
    with pytest.raises(ValueError, match="one label in 0..255 per region channel"):
        ops.region_labels(x, (1, 256))
