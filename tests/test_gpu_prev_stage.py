"""cf_prev_stage_onehot (csrc/prev_stage.hip): batchgenerators' resize_segmentation(order=1) + nnU-Net's to_one_hot in one kernel, written
straight into the network-input tensor.  Expected planes: oracle.preprocess.resize_segmentation (float64, scipy) plus a three-line
one-hot, computed once per case on the CPU and shared by the tests.  Every comparison is bit-exact equality of all planes.

Condition on the inputs of THIS file (asserted below with the oracle alone, before the GPU is touched): over every label present, the
resized float64 indicator stays at least TIE_MARGIN = 1e-4 away from 0.5, so no voxel's label depends on rounding and the rows test
the kernel's shape handling (tails, alignment, classes, offsets) whatever its arithmetic.  The cases marked `exact` need no margin:
every per-axis weight is a dyadic fraction with at most 3 fractional bits (shape ratios 2, 1/2), so all products and sums are exact
in any precision and order -- there the `>=` itself, indicators of exactly 0.5 included, must agree with the oracle.
Indicators of exactly 0.5 with weights that round are NOT implementation-defined: the reference's side is that of one fixed float64
chain, the kernel runs that chain, and tests/test_gpu_label_resize.py holds it to the oracle on maps chosen for such ties.

Label maps: seeded Gaussian-smoothed noise quantised to equal-volume labels; the seeds were picked on the CPU for the margin."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIE_MARGIN = 1e-4
# name: (source shape, output shape, seed, labels in the map, classes, exact)
CASES = {
    "odd_z2_multiple_of_4": ((5, 9, 7), (8, 20, 12), 1, 4, [1, 2, 3], False),       # 480 four-voxel units: two blocks
    "doubling": ((4, 6, 6), (8, 12, 12), 1, 4, [1, 2, 3], False),
    "one_axis_unchanged": ((5, 9, 7), (5, 20, 12), 1, 4, [1, 2, 3], False),
    "identity": ((5, 9, 7), (5, 9, 7), 1, 4, [1, 2, 3], False),
    "scalar_tail": ((5, 9, 7), (8, 20, 13), 8, 4, [1, 2, 3], False),                # Z2 % 4 == 1; rows start off the 16-byte grid
    "labels_outside_classes": ((5, 9, 7), (8, 20, 12), 12, 6, [1, 2, 3], False),    # labels 0..5: 4 and 5 compete and get no plane
    "classes_out_of_order": ((5, 9, 7), (8, 20, 12), 1, 4, [3, 1], False),
    "halving_exact_ties": ((8, 8, 8), (4, 4, 4), 1, 4, [1, 2, 3], True),           # every weight 1/2: indicators of exactly 0.5 occur
    "grid_stride": ((64, 64, 66), (128, 128, 132), 2, 4, [1, 2, 3], True),          # 540 672 units > 2048 blocks x 256 threads
}


def smoothed_labels(shape, seed, nlabels):
    from scipy.ndimage import gaussian_filter
    g = gaussian_filter(np.random.RandomState(seed).randn(*shape), 1.5)
    return np.digitize(g, np.quantile(g, np.linspace(0, 1, nlabels + 1)[1:-1])).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    """(seg uint8, expected planes float32 [len(classes), *dst], min |indicator - 0.5|, #indicators == 0.5) -- oracle only, computed once"""
    from oracle import preprocess as OP
    src, dst, seed, nlabels, classes, _exact = CASES[name]
    seg = smoothed_labels(src, seed, nlabels)
    assert len(np.unique(seg)) == nlabels
    inds = [OP.resize((seg == c).astype(float), dst, 1, mode="edge", clip=True, anti_aliasing=False) for c in np.unique(seg)]
    margin = min(float(np.abs(i - 0.5).min()) for i in inds)
    ties = sum(int((i == 0.5).sum()) for i in inds)
    resized = OP.resize_segmentation(seg, dst, order=1)
    expected = np.zeros((len(classes),) + tuple(dst), dtype=np.float32)
    for j, c in enumerate(classes):
        expected[j][resized == c] = 1
    for a in (seg, expected):
        a.setflags(write=False)
    return seg, expected, margin, ties


def fused(dev, seg, dst, classes):
    from cineflow import ops
    out = torch.full((len(classes),) + tuple(dst), 7.0, dtype=torch.float32, device=dev)
    ops.prev_stage_onehot(torch.tensor(seg).to(dev), classes, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_oracle_bit_for_bit(dev, name):
    src, dst, _seed, _n, classes, exact = CASES[name]
    seg, expected, margin, ties = case(name)
    print("%s: min |indicator - 0.5| = %.3e, indicators == 0.5: %d, unlabelled output %.3f"
          % (name, margin, ties, float((expected.sum(0) == 0).mean())))
    if exact:
        if name == "halving_exact_ties":
            assert ties > 0, "no indicator is exactly 0.5: the case does not test the >= itself"
    else:
        assert margin >= TIE_MARGIN, "the input violates the tie condition: min |indicator - 0.5| = %.3e" % margin
    got = fused(dev, seg, dst, classes)
    assert np.array_equal(got, expected), "%d of %d plane values differ" % (int((got != expected).sum()), expected.size)


def test_voxels_without_a_label_at_one_half_are_background():
    """the property the planes must keep: where three or more labels meet no indicator reaches 0.5 and the oracle leaves 0"""
    from oracle import preprocess as OP
    seg, expected, _m, _t = case("odd_z2_multiple_of_4")
    dst = CASES["odd_z2_multiple_of_4"][1]
    inds = np.stack([OP.resize((seg == c).astype(float), dst, 1, mode="edge", clip=True, anti_aliasing=False) for c in range(4)])
    none = (inds < 0.5).all(0)
    assert none.mean() > 0.01 and not expected[:, none].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_the_unfused_route(dev, name):
    """to_one_hot(_resize_labels(...)): one cf_resize_labels launch, then a compare per class"""
    from cineflow import preprocessing as P
    _src, dst, _seed, _n, classes, _exact = CASES[name]
    seg, expected, _m, _t = case(name)
    t = torch.tensor(seg).to(dev)
    labels = P._resize_labels(t[None].float(), dst, [1, 1, 1])[0]
    unfused = P.to_one_hot(labels, classes)
    assert unfused.dtype == torch.float32 and tuple(unfused.shape) == expected.shape
    assert np.array_equal(unfused.cpu().numpy(), fused(dev, seg, dst, classes))


@pytest.mark.parametrize("name", ["odd_z2_multiple_of_4", "scalar_tail"])
def test_planes_are_written_in_place_and_nothing_else(dev, name):
    """channels 1..3 of a [4, ...] network input inside one larger allocation: channel 0 and the guard behind the last plane stay"""
    from cineflow import ops
    _src, dst, _seed, _n, classes, _exact = CASES[name]
    seg, expected, _m, _t = case(name)
    V2, guard = int(np.prod(dst)), 64
    buf = torch.full((4 * V2 + guard,), 7.0, dtype=torch.float32, device=dev)
    x = buf[:4 * V2].view(4, *dst)
    ch0 = torch.randn(dst, generator=torch.Generator().manual_seed(3))
    x[0].copy_(ch0)
    ret = ops.prev_stage_onehot(torch.tensor(seg).to(dev), classes, x[1:])
    assert ret.data_ptr() == x[1:].data_ptr()
    host = buf.cpu()
    assert torch.equal(host[:V2].view(dst), ch0), "channel 0 was touched"
    assert bool((host[4 * V2:] == 7.0).all()), "the kernel wrote past the last plane"
    assert np.array_equal(host[V2:4 * V2].view(3, *dst).numpy(), expected)


def test_python_layers_match_the_oracle(dev):
    """preprocessing.resize_segmentation / to_one_hot / prev_stage_to_input: numpy in, numpy out, the reference's dtypes"""
    from cineflow import preprocessing as P
    from oracle import preprocess as OP
    src, dst, _seed, _n, classes, _exact = CASES["odd_z2_multiple_of_4"]
    seg, expected, _m, _t = case("odd_z2_multiple_of_4")
    r = P.resize_segmentation(seg.astype(np.int16), dst, order=1)
    assert r.dtype == np.int16 and np.array_equal(r, OP.resize_segmentation(seg, dst, 1))
    r2 = P.resize_segmentation(seg[2], (20, 12), order=1)                            # a 2-D map
    assert np.array_equal(r2, OP.resize_segmentation(seg[2], (20, 12), 1))
    oh = P.to_one_hot(r, classes)
    assert oh.dtype == np.int16 and np.array_equal(oh.astype(np.float32), expected)
    assert np.array_equal(P.to_one_hot(r), P.to_one_hot(r, [0, 1, 2, 3]))
    data = torch.randn(2, *dst, generator=torch.Generator().manual_seed(4)).numpy()
    x = P.prev_stage_to_input(data, seg.astype(np.int64), classes)
    assert x.dtype == np.float32 and x.shape == (5,) + tuple(dst)
    assert np.array_equal(x[:2], data) and np.array_equal(x[2:], expected)
    with pytest.raises(ValueError, match="0..255"):
        P.prev_stage_to_input(data, seg.astype(np.int64) + 300, classes)


def test_offsets_past_2_31_bytes(dev):
    """Three planes of 256 x 700 x 1024 voxels are 2.2e9 bytes: the last plane straddles byte 2^31.  The source is two slabs (label 1,
    then label 3) along the first axis, so the expected planes need no oracle run: with s = (i + 0.5) / 128 - 0.5 label 1's indicator
    is 1 - s >= 0.5 for i <= 127 and label 3's is s > 0.5 for i >= 128 (s = 0.5 needs i = 127.5: no tie), the other axes are constant."""
    from cineflow import ops
    seg = torch.ones((2, 2, 2), dtype=torch.uint8, device=dev)
    seg[1] = 3
    dst = (256, 700, 1024)
    assert 3 * int(np.prod(dst)) * 4 > 2 ** 31 and 2 * int(np.prod(dst)) * 4 < 2 ** 31
    out = torch.full((3,) + dst, 7.0, dtype=torch.float32, device=dev)
    ops.prev_stage_onehot(seg, [1, 2, 3], out)
    assert float(out[0, :128].min()) == 1.0 and float(out[0, 128:].max()) == 0.0
    assert float(out[1].min()) == 0.0 and float(out[1].max()) == 0.0
    assert float(out[2, :128].max()) == 0.0 and float(out[2, 128:].min()) == 1.0
