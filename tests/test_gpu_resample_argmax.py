"""cf_resample_argmax (csrc/postprocess.hip) through cineflow.ops.resample_argmax on the device, held bit for bit to the composition of
what exists, none of which is the code under test:

  * the resampled channels: ops.resize3d (cf_resize3d, itself pinned to the reference's resampling);
  * the labels: numpy's argmax(0), or the region loop of segmentation_export.py:148-150, placed into zeros of the full volume;
  * the stored probabilities: export.probabilities_as_stored (numpy's astype(float16), and the regions' nudge above 0.5);
  * the counts: metrics.label_histogram (cf_label_confusion) at K = 16 on the composed label volume.

Shapes are the smallest at which the kernel can go wrong: odd sizes, both directions and equal sizes, a source axis of length 1, the two
separate-z flag sets, a crop inside a larger volume, and one volume with more voxels than one trip of the grid covers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIST_K = 16


def _src(shape, seed, band=None):
    g = np.random.default_rng(seed)
    if band is not None:                                               # region probabilities crowded around 0.5: the nudge interval gets hit
        return (0.5 + (g.random(shape, dtype=np.float32) - 0.5) * band).astype(np.float32)
    return g.random(shape, dtype=np.float32)


def _gt(full, seed, high=4):
    return np.random.default_rng(seed).integers(0, high, size=full, dtype=np.uint8)


def composed(src, new_shape, linear, full, lo, order, gt, dev):
    """(labels in the full volume, stored fp16 probabilities, hist [16,16], overflow count) by the existing route"""
    from cineflow import export, metrics, ops
    res = ops.resize3d(torch.from_numpy(src).to(dev), new_shape, linear).cpu().numpy()
    if order is None:
        lab = res.argmax(0)
    else:
        lab = np.zeros(res.shape[1:])
        for i, c in enumerate(order):
            lab[res[i] > 0.5] = c
    seg = np.zeros(full, dtype=np.uint8)
    seg[tuple(slice(a, a + n) for a, n in zip(lo, new_shape))] = lab
    stored = export.probabilities_as_stored(res, order)
    hist, overflow = metrics.label_histogram(torch.from_numpy(seg).to(dev), torch.from_numpy(gt).to(dev), HIST_K)
    return seg, stored, hist, overflow, res


def check(src, new_shape, linear, full=None, lo=(0, 0, 0), order=None, gt_high=4, dev=None):
    from cineflow import ops
    full = tuple(new_shape) if full is None else full
    gt = _gt(full, 99, gt_high)
    want_seg, want_probs, want_hist, want_over, res = composed(src, new_shape, linear, full, lo, order, gt, dev)
    seg, probs, hist = ops.resample_argmax(torch.from_numpy(src).to(dev), new_shape, linear, full_shape=full, bbox_lo=lo,
                                           regions_class_order=order, want_probs=True, gt=torch.from_numpy(gt).to(dev))
    torch.cuda.synchronize()
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == full
    assert probs.dtype == torch.float16 and tuple(probs.shape) == (src.shape[0],) + tuple(new_shape)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (HIST_K * HIST_K + 1,)
    seg, probs, hist = seg.cpu().numpy(), probs.cpu().numpy(), hist.cpu().numpy()
    assert np.array_equal(seg, want_seg), "labels differ at %d voxels" % int((seg != want_seg).sum())
    assert np.array_equal(probs.view(np.uint16), want_probs.view(np.uint16)), "stored probabilities differ"
    assert np.array_equal(hist[:-1].reshape(HIST_K, HIST_K), want_hist) and int(hist[-1]) == want_over
    assert int(hist.sum()) == int(np.prod(full))                       # every voxel of the full volume is counted once, the margin included
    # the optional outputs change nothing
    seg_only, none_p, none_h = ops.resample_argmax(torch.from_numpy(src).to(dev), new_shape, linear, full_shape=full, bbox_lo=lo,
                                                   regions_class_order=order)
    assert none_p is None and none_h is None and np.array_equal(seg_only.cpu().numpy(), want_seg)
    return seg, probs, hist, res


CASES = {
    # name: (K, source, target, linear, full, lo)
    "up_in_box": (3, (5, 7, 6), (9, 12, 11), (1, 1, 1), (11, 12, 14), (1, 0, 2)),
    "down": (4, (9, 12, 11), (5, 7, 6), (1, 1, 1), None, (0, 0, 0)),
    "equal": (4, (5, 7, 6), (5, 7, 6), (1, 1, 1), None, (0, 0, 0)),
    "one_channel": (1, (5, 7, 6), (9, 12, 11), (1, 1, 1), (10, 13, 11), (1, 0, 0)),
    "axis_of_one": (3, (1, 7, 6), (4, 9, 8), (1, 1, 1), None, (0, 0, 0)),
    "separate_first": (3, (5, 7, 6), (9, 12, 11), (0, 1, 1), (11, 12, 14), (1, 0, 2)),
    "separate_last": (4, (9, 12, 11), (5, 7, 6), (1, 1, 0), (6, 9, 9), (1, 0, 2)),
    "nearest": (3, (5, 7, 6), (9, 12, 11), (0, 0, 0), None, (0, 0, 0)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_softmax_cases_equal_the_composed_route(dev, name):
    K, shape, new_shape, linear, full, lo = CASES[name]
    seg, _probs, hist, _res = check(_src((K,) + shape, 3), new_shape, linear, full, lo, dev=dev)
    if full is not None:                                               # outside the box: zeros, and counted
        inside = np.zeros(full, dtype=bool)
        inside[tuple(slice(a, a + n) for a, n in zip(lo, new_shape))] = True
        assert not seg[~inside].any() and int(hist[:HIST_K].sum()) >= int((~inside).sum())
    if K > 1:
        assert len(np.unique(seg)) > 1, "one label everywhere: the check would be vacuous"


@pytest.mark.parametrize("name", ["up_in_box", "down", "equal", "separate_first", "separate_last"])
def test_region_cases_equal_the_composed_route(dev, name):
    K, shape, new_shape, linear, full, lo = CASES[name]
    order = [1, 3, 2, 1][:K]
    seg, probs, _hist, res = check(_src((K,) + shape, 5, band=2.0 ** -9), new_shape, linear, full, lo, order=order, dev=dev)
    nudged = (res > 0.5) & (res.astype(np.float16) <= np.float16(0.5))
    assert nudged.sum() > 0, "no value in (0.5, 0.5 + 2^-12]: the nudge would go unchecked"
    assert np.all(probs[nudged].view(np.uint16) == 0x3801)
    assert np.array_equal(probs > np.float16(0.5), res > 0.5)           # the stored member says what the label file says


def test_second_trip_of_the_grid(dev):
    """more voxels than 8 blocks of 256 threads per compute unit cover at once, and no multiple of 256"""
    full = (81, 83, 89)
    voxels = int(np.prod(full))
    assert voxels % 256 and voxels > 256 * 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    check(_src((4, 30, 35, 33), 7), (79, 83, 86), (0, 1, 1), full, (2, 0, 3), dev=dev)


def test_the_first_of_equal_maxima_wins(dev):
    src = _src((4, 5, 7, 6), 11) * 0.5
    src[1] = src[2] = 0.75 + src[3] * 0.25                             # two identical channels above the others, almost everywhere
    for new_shape in ((5, 7, 6), (9, 12, 11)):
        seg, _p, _h, _r = check(src, new_shape, (1, 1, 1), dev=dev)
        assert (seg == 1).any() and not (seg == 2).any()
    same = np.full((3, 4, 5, 6), 0.25, dtype=np.float32)               # all channels equal: label 0
    assert not check(same, (7, 5, 9), (1, 1, 1), dev=dev)[0].any()


def test_region_thresholds_and_small_values(dev):
    """at equal sizes the kernel copies, so the stored values are the planted ones"""
    shape = (4, 6, 8)
    src = _src((3,) + shape, 13) * 0.4                                 # nothing above 0.5 but what is planted
    planted = [0.5, 0.5 + 2.0 ** -13, 0.5 + 2.0 ** -12, 0.5 + 2.0 ** -12 + 2.0 ** -20, 0.5 + 2.0 ** -11, np.nextafter(np.float32(0.5), np.float32(1)),
               6.0e-5, 6.2e-5, 1.0e-6, 3.1e-8, 2.9e-8, 2.0 ** -25, 2.0 ** -24, 1.0e-12, 0.0, -1.0e-7, 1.0]
    for k in range(3):
        src[k].reshape(-1)[k:k + 2 * len(planted):2] = np.asarray(planted, dtype=np.float32)
    order = [2, 1, 3]
    seg, probs, _hist, _res = check(src, shape, (1, 1, 1), order=order, dev=dev)
    flat_seg, flat_p = seg.reshape(-1), probs[0].reshape(-1)
    assert flat_seg[0] == 0 and flat_p[0] == np.float16(0.5)           # exactly 0.5 paints nothing and stays 0.5
    assert flat_p[2].view(np.uint16) == 0x3801 and flat_p[4].view(np.uint16) == 0x3801 and flat_seg[2] != 0
    assert np.any((probs != 0) & (np.abs(probs.astype(np.float32)) < 2.0 ** -14)), "no fp16 subnormal was stored"
    check(src, shape, (1, 1, 1), dev=dev)                              # and the same planted values through the arg-max


def test_labels_of_16_and_more_go_to_the_last_bin(dev):
    src = _src((3, 5, 7, 6), 17, band=0.5)
    _seg, _p, hist, _r = check(src, (9, 12, 11), (1, 1, 1), (10, 12, 13), (0, 0, 1), order=[1, 2, 20], dev=dev)
    assert hist[-1] > 0
    _seg, _p, hist, _r = check(_src((3, 5, 7, 6), 19), (9, 12, 11), (1, 1, 1), gt_high=19, dev=dev)      # the ground truth's side
    assert hist[-1] > 0


def test_argument_refusals(dev):
    from cineflow import ops
    ok = torch.zeros((3, 5, 7, 6), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="0 classes"):
        ops.resample_argmax(torch.zeros((0, 5, 7, 6), dtype=torch.float32, device=dev), (5, 7, 6), (1, 1, 1))
    with pytest.raises(ValueError, match="256 classes"):
        ops.resample_argmax(torch.zeros((256, 2, 2, 2), dtype=torch.float32, device=dev), (2, 2, 2), (1, 1, 1))
    with pytest.raises(ValueError, match="do not fit"):
        ops.resample_argmax(ok, (9, 12, 11), (1, 1, 1), full_shape=(10, 12, 11), bbox_lo=(2, 0, 0))
    with pytest.raises(ValueError, match="do not fit"):
        ops.resample_argmax(ok, (9, 12, 11), (1, 1, 1), full_shape=(10, 12, 11), bbox_lo=(0, -1, 0))
    with pytest.raises(ValueError, match="contiguous"):
        ops.resample_argmax(torch.zeros((3, 5, 6, 7), dtype=torch.float32, device=dev).transpose(2, 3), (5, 7, 6), (1, 1, 1))
    with pytest.raises(ValueError, match="gt must be"):
        ops.resample_argmax(ok, (9, 12, 11), (1, 1, 1), gt=torch.zeros((9, 12, 10), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="gt must be"):
        ops.resample_argmax(ok, (9, 12, 11), (1, 1, 1), full_shape=(10, 12, 11), gt=torch.zeros((9, 12, 11), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="float32"):
        ops.resample_argmax(ok.half(), (9, 12, 11), (1, 1, 1))
    with pytest.raises(TypeError):
        ops.resample_argmax(ok.cpu(), (9, 12, 11), (1, 1, 1))
    with pytest.raises(ValueError, match="one label in 0..255 per region channel"):
        ops.resample_argmax(ok, (9, 12, 11), (1, 1, 1), regions_class_order=[1, 2])


def test_the_library_refuses_on_the_host():
    """the entry point's own checks; every call is refused before a launch and no pointer is dereferenced"""
    from cineflow import _lib
    h = _lib.lib()
    PTR = 0x1000

    def call(K=3, src=(5, 7, 6), new=(9, 12, 11), full=(9, 12, 11), lo=(0, 0, 0), gt=None, hist=None):
        return h.cf_resample_argmax(PTR, K, *src, *new, 1, 1, 1, PTR, *full, *lo, None, None, gt, hist, None)

    for kwargs, text in ((dict(K=0), b"K = 0 is outside 1..255"), (dict(K=256), b"K = 256 is outside 1..255"),
                         (dict(lo=(0, 0, 1)), b"the crop (9, 12, 11) at (0, 0, 1) overhangs the volume (9, 12, 11)"),
                         (dict(new=(9, 0, 11)), b"bad shape"), (dict(gt=PTR), b"gt and hist go together"), (dict(hist=PTR), b"gt and hist go together")):
        rc = call(**kwargs)
        assert rc != 0 and h.cf_last_error().startswith(b"cf_resample_argmax: ") and text in h.cf_last_error(), (kwargs, rc, h.cf_last_error())
    assert h.cf_resample_argmax(None, 3, 5, 7, 6, 9, 12, 11, 1, 1, 1, PTR, 9, 12, 11, 0, 0, 0, None, None, None, None, None) != 0
