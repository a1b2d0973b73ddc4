"""MTLmodel as the segmentation network of a device batch: MTLmodel.accumulate_tta_batch (one cropper forward, cf_crop_windows, one
cf_tile_gather, one network call per flip at B, cf_tta_accumulate_window) against the oracle's per-sample statement of
MTL_model.py:816-936 and against MTLmodel.mirror_and_predict_2d, at the project's MTLmodel bound of 5e-5 (tests/test_mtl.py).

Reduced width, image 96, crop 64, window 8, B = 5: three structured samples, one all-zero, one constant.  The cropper's label maps
decide the windows, so the seeds are chosen on the CPU such that the oracle's float32 and float64 label maps are equal at every pixel
and the smallest top-two logit gap of the cropper (float64) is at least 1e-3 -- 20 times the bound, so no label and hence no window can
flip on the device.  Cropper seed 73, input seed 106; per sample the smallest gap is
    sample 0: 1.631e-03   sample 1: 1.333e-01   sample 2: 7.285e-02   sample 3: all-zero (the network is not consulted)   sample 4: 1.767e-01
(printed and asserted again by the first test) and the windows are (0, 64, 32, 96), (16, 80, 16, 80), (0, 64, 0, 64), (16, 80, 16, 80),
(16, 80, 16, 80): a corner, a border and the centre."""
import pytest
import torch

import _mtl_oracle as MO

pytestmark = pytest.mark.gpu

CROP_SEED, SEG_SEEDS, X_SEED = 73, (74, 76), 106
BOUND = 5e-5
_cache = {}


def _batch():
    x = MO.smooth_images(5, MO.IMAGE, MO.IMAGE, X_SEED)
    x[3] = 0.0
    x[4] = 0.5
    return x


def _oracle(normalize):
    """the oracle's per-sample softmax of both folds and its windows, computed once per setting"""
    key = ("oracle", normalize)
    if key not in _cache:
        if "nets" not in _cache:
            _cache["nets"] = MO.oracle_nets(CROP_SEED, SEG_SEEDS)
        ocrop, osegs = _cache["nets"]
        res = [MO.oracle_wrapper(ocrop, o, _batch(), normalize) for o in osegs]
        _cache[key] = ([r[0] for r in res], res[0][1])
    return _cache[key]


def _device_nets(dev, normalize=False):
    from cineflow.inference import Processor
    from cineflow.mtl import MTLmodel
    from cineflow.weights import seeded_state_dict
    if "dev" not in _cache:
        crop = MTLmodel(MO.IMAGE, MO.WINDOW, 2, **MO.RED)
        crop.load_state_dict(seeded_state_dict(crop.state_shapes(), CROP_SEED), dev)
        proc = Processor(MO.CROP, MO.IMAGE, crop)
        segs = []
        for s in SEG_SEEDS:
            m = MTLmodel(MO.CROP, MO.WINDOW, 4, processor=proc, **MO.RED)
            segs.append(m.load_state_dict(seeded_state_dict(m.state_shapes(), s), dev))
        _cache["dev"] = (crop, segs)
    crop, segs = _cache["dev"]
    for m in segs:
        m.normalize = normalize
    return crop, segs


def test_the_seeds_leave_the_cropper_no_label_to_flip():
    """CPU side of the setup: float32 and float64 label maps of the oracle's cropper are equal, the smallest top-two gap is >= 1e-3"""
    ocrop, _ = MO.oracle_nets(CROP_SEED, ())
    ocrop64, _ = MO.oracle_nets(CROP_SEED, (), torch.float64)
    x = _batch()
    l32, l64 = MO.cropper_logits(ocrop, x), MO.cropper_logits(ocrop64, x)
    assert l32[3] is None and l64[3] is None
    for b in (0, 1, 2, 4):
        gap = float(MO.top_two_gap(l64[b]).min())
        print("sample %d: smallest top-two logit gap of the cropper %.3e" % (b, gap))
        assert gap >= 1e-3, (b, gap)
        assert torch.equal(l32[b].argmax(1), l64[b].argmax(1)), b
    assert len({tuple(w) for w in _oracle(False)[1]}) >= 3, "the samples should not all share one window"


def test_windows_equal_the_oracles_per_sample_windows(dev):
    _crop, segs = _device_nets(dev)
    win, jobs = segs[0].crop_windows_of(_batch().to(dev))
    want = _oracle(False)[1]
    assert win.cpu().tolist() == want
    assert jobs.cpu().tolist() == [[b, w[2], w[0]] for b, w in enumerate(want)]


@pytest.mark.parametrize("normalize", (False, True))
def test_batched_wrapper_vs_oracle_and_vs_the_per_sample_wrapper(dev, normalize):
    _crop, segs = _device_nets(dev, normalize)
    x = _batch().to(dev)
    want = _oracle(normalize)[0][0]
    acc = torch.zeros(5, 4, MO.IMAGE, MO.IMAGE, device=dev)
    segs[0].accumulate_tta_batch(x, acc, 0.25)                                   # normalize=None: the model's own attribute
    d_oracle = float((acc.cpu() - want).abs().max())
    per_sample = segs[0].mirror_and_predict_2d(x, normalize=normalize)
    d_sample = float((acc - per_sample).abs().max())
    d_sample_oracle = float((per_sample.cpu() - want).abs().max())
    print("normalize=%s: batched vs oracle %.3e, batched vs per-sample wrapper %.3e (per-sample vs oracle %.3e)" % (normalize, d_oracle, d_sample, d_sample_oracle))
    assert bool(torch.isfinite(acc).all())
    assert d_oracle <= BOUND, d_oracle
    assert d_sample <= BOUND, d_sample
    for b, (x0, _x1, y0, _y1) in enumerate(_oracle(normalize)[1]):               # zero outside the window, a distribution inside
        inside = torch.zeros(MO.IMAGE, MO.IMAGE, dtype=torch.bool, device=dev)
        inside[y0:y0 + MO.CROP, x0:x0 + MO.CROP] = True
        assert float(acc[b][:, ~inside].abs().max()) == 0.0, b
        assert float((acc[b][:, inside].sum(0) - 1.0).abs().max()) <= 1e-5, b


def test_without_a_processor_it_is_mirror_and_predict_2d(dev):
    from cineflow.inference import mirror_and_predict_2d
    from cineflow.mtl import MTLmodel, _LogitsOf
    from cineflow.weights import seeded_state_dict
    m = MTLmodel(MO.CROP, MO.WINDOW, 4, **MO.RED)
    m.load_state_dict(seeded_state_dict(m.state_shapes(), SEG_SEEDS[0]), dev)
    x = MO.smooth_images(3, MO.CROP, MO.CROP, 9).to(dev)
    acc = torch.zeros(3, 4, MO.CROP, MO.CROP, device=dev)
    assert m.accumulate_tta_batch(x, acc, 0.25) is None
    assert torch.equal(acc, mirror_and_predict_2d(_LogitsOf(m), x))


@pytest.mark.parametrize("normalize", (False, True))
def test_fold_ensemble_one_cropper_forward_per_batch_and_shared_windows(dev, normalize):
    """ensemble_predict_2d on two folds: ONE cropper forward at B, flips x folds segmenter forwards at B, the windows computed once and
    handed to the second fold; the softmax is the oracle's fold mean"""
    from cineflow.inference import ensemble_predict_2d
    crop, segs = _device_nets(dev, normalize)
    calls = {"crop": [], "seg": [], "windows": []}
    undo = []

    def count(net, key):
        inner = net.forward

        def forward(x):
            calls[key].append(int(x.shape[0]))
            return inner(x)
        net.forward = forward
        undo.append(net)

    count(crop, "crop")
    for m in segs:
        count(m, "seg")
        inner = m.accumulate_tta_batch

        def acc_batch(*a, _inner=inner, **k):
            calls["windows"].append(k.get("windows"))
            out = _inner(*a, **k)
            calls["windows"].append(out)
            return out
        m.accumulate_tta_batch = acc_batch
    try:
        got = ensemble_predict_2d(segs, _batch().to(dev))
    finally:
        for net in undo:
            del net.forward
        for m in segs:
            del m.accumulate_tta_batch
    assert calls["crop"] == [5], calls["crop"]
    assert calls["seg"] == [5] * (4 * len(segs)), calls["seg"]
    given0, made0, given1, made1 = calls["windows"]
    assert given0 is None and given1 is made0 and made1 is made0                 # the second fold received the first fold's tables
    assert made0[0].cpu().tolist() == _oracle(normalize)[1]
    want = sum(_oracle(normalize)[0]) / len(segs)
    d = float((got.cpu() - want).abs().max())
    print("two folds, normalize=%s: ensemble vs the oracle's fold mean %.3e" % (normalize, d))
    assert d <= BOUND, d
