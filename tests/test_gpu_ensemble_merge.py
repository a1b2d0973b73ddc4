"""cf_ensemble_merge (csrc/ensemble.hip), cineflow.ops.ensemble_merge and cineflow.ensemble_predictions on the device.

Expected values are this file's own numpy statement of what nnunet/inference/ensemble_predictions.py runs: np.mean(np.vstack([a[None] for a
in members]), 0), argmax(0) (or the regions_class_order overwrite loop of segmentation_export.py) and the bounding-box placement into zeros.
Every comparison is bit for bit -- labels as uint8, means as raw bits -- and there is no tolerance anywhere.  The expected arrays are computed
once per case on the CPU, shared by the tests and write-protected.

Members are seeded softmaxes over K of 2 N(0,1) logits, rounded to fp16 (and widened to fp32 for the fp32 runs, so that both dtypes see the
same numbers).  Two CPU guards make sure these inputs can tell the stated arithmetic from its two near misses: with N = 7 at least one element
where s * (1 / N) rounds differently from s / N, and with N = 3 at least one voxel where the arg-max of the fp32 sum is not the arg-max of
the fp16 mean.

Volumes past 2^31 elements are not tested (they do not fit a test of seconds): the 64-bit offsets are checked by review only."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0
# name: (member shape [K,Z,Y,X], volume before cropping or None, where the crop goes)
SHAPES = {
    "main": ((4, 5, 13, 17), (7, 16, 24), (1, 2, 3)),       # unaligned rows, a row tail, an odd x offset, margins on every side; 3 blocks
    "aligned": ((4, 3, 8, 16), None, (0, 0, 0)),            # every load and store takes the wide path
    "nine": ((2, 1, 1, 9), None, (0, 0, 0)),                # one whole chunk and a one-voxel tail
    "x0_8": ((5, 2, 3, 8), (2, 3, 24), (0, 0, 8)),          # whole aligned chunks between two whole margin chunks
}
NS = (1, 2, 3, 7)
DTYPES = {"fp16": np.float16, "fp32": np.float32}


def softmax_members(shape, n, seed=SEED, scale=2.0):
    rng = np.random.default_rng(seed)
    logits = scale * rng.standard_normal((n,) + tuple(shape))
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float16)


def numpy_merge(members, full=None, lo=(0, 0, 0), order=None):
    """the reference's arithmetic -> (labels uint8 [Zf,Yf,Xf], mean [K,Z,Y,X])"""
    mean = np.mean(np.vstack([a[None] for a in members]), 0)
    if order is None:
        seg = mean.argmax(0)
    else:
        seg = np.zeros(mean.shape[1:])
        for i, c in enumerate(order):
            seg[mean[i] > 0.5] = c
    full = tuple(seg.shape) if full is None else tuple(full)
    out = np.zeros(full, dtype=np.uint8)
    out[tuple(slice(a, a + n) for a, n in zip(lo, seg.shape))] = seg
    assert mean.dtype == members[0].dtype
    return out, mean


@functools.lru_cache(maxsize=None)
def case(name, n, dtype):
    shape, full, lo = SHAPES[name]
    members = [m.astype(DTYPES[dtype]) for m in softmax_members(shape, n)]
    seg, mean = numpy_merge(members, full, lo)
    for a in members + [seg, mean]:
        a.setflags(write=False)
    return members, seg, mean


def bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def run(dev, members, full=None, lo=(0, 0, 0), want_mean=True, order=None):
    from cineflow import ops
    seg, mean = ops.ensemble_merge([torch.from_numpy(np.array(m)).to(dev) for m in members], full, lo, want_mean=want_mean,
                                   regions_class_order=order)
    assert seg.dtype == torch.uint8 and (mean is None) == (not want_mean)
    return seg.cpu().numpy(), None if mean is None else mean.cpu().numpy()


def test_the_seeded_inputs_can_tell_the_arithmetic_from_its_near_misses():
    """CPU only.  If either assertion fails, pick another SEED; the checks below stay as they are."""
    m7 = np.stack(case("main", 7, "fp16")[0]).astype(np.float32)
    s = m7[0].copy()
    for a in m7[1:]:
        s = s + a
    assert s.dtype == np.float32
    by_div = (s / np.float32(7)).astype(np.float16)
    by_mul = (s * (np.float32(1) / np.float32(7))).astype(np.float16)
    assert np.array_equal(bits(by_div), bits(case("main", 7, "fp16")[2])), "the sequential fp32 sum and division is not numpy's mean"
    ndiff = int((bits(by_div) != bits(by_mul)).sum())
    print("N = 7: s * (1 / N) rounds differently from s / N in %d of %d elements" % (ndiff, by_div.size))
    assert ndiff >= 1
    m3 = np.stack(case("main", 3, "fp16")[0]).astype(np.float32)
    s3 = (m3[0] + m3[1]) + m3[2]
    of_sum, of_mean = s3.argmax(0), case("main", 3, "fp16")[2].argmax(0)
    nvox = int((of_sum != of_mean).sum())
    print("N = 3: arg-max of the fp32 sum differs from arg-max of the fp16 mean in %d of %d voxels" % (nvox, of_sum.size))
    assert nvox >= 1


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_equals_numpy_bit_for_bit(dev, name, n, dtype):
    _shape, full, lo = SHAPES[name]
    members, seg, mean = case(name, n, dtype)
    got_seg, got_mean = run(dev, members, full, lo)
    assert got_seg.shape == seg.shape and got_mean.shape == mean.shape and got_mean.dtype == mean.dtype
    assert np.array_equal(bits(got_mean), bits(mean)), "%d of %d mean values differ in their bits" % (int((bits(got_mean) != bits(mean)).sum()), mean.size)
    assert np.array_equal(got_seg, seg), "%d of %d labels differ" % (int((got_seg != seg).sum()), seg.size)
    only_seg, none = run(dev, members, full, lo, want_mean=False)
    assert none is None and np.array_equal(only_seg, seg)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_ties_go_to_the_first_maximum(dev, dtype):
    shape, full, lo = SHAPES["main"]
    members = [(np.round(m.astype(np.float32) * 2) / 2).astype(DTYPES[dtype]) for m in softmax_members(shape, 3, seed=SEED + 1)]
    seg, mean = numpy_merge(members, full, lo)
    tied = float(((mean == mean.max(0)).sum(0) > 1).mean())
    print("the top class is tied in %.1f %% of the voxels" % (100 * tied))
    assert tied > 0.1
    got_seg, got_mean = run(dev, members, full, lo)
    assert np.array_equal(bits(got_mean), bits(mean)) and np.array_equal(got_seg, seg)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_small_probabilities_keep_their_subnormal_bits(dev, dtype):
    """Saved fp16 softmaxes hold subnormal values (below 6.1e-5) wherever a class is unlikely; with logits of 8 N(0,1) a fifth of the main
    shape's values are, and so are many of the means.  The fp32 run scales them by 2^-120 -- exact: a power of two, and no result passes
    below fp32's smallest subnormal 2^-149 -- so that its sums and quotients are subnormal fp32."""
    shape, full, lo = SHAPES["main"]
    members = softmax_members(shape, 3, scale=8.0)
    if dtype == "fp32":
        members = [m.astype(np.float32) * np.float32(2.0 ** -120) for m in members]
        tiny = np.float32(2.0 ** -126)
    else:
        members = list(members)
        tiny = np.float16(2.0 ** -14)
    seg, mean = numpy_merge(members, full, lo)
    sub = float(((mean > 0) & (mean < tiny)).mean())
    print("%.1f %% of the means are subnormal" % (100 * sub))
    assert sub > 0.05
    got_seg, got_mean = run(dev, members, full, lo)
    assert np.array_equal(bits(got_mean), bits(mean)) and np.array_equal(got_seg, seg)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_regions_class_order_overwrites_in_order(dev, dtype):
    """three independent region probabilities per voxel (not a softmax): regions overlap, and some voxels belong to none"""
    shape, full, lo = (3, 5, 13, 17), (7, 16, 24), (1, 2, 3)
    rng = np.random.default_rng(SEED + 2)
    members = [rng.random(shape).astype(np.float16).astype(DTYPES[dtype]) for _ in range(3)]
    order = (3, 1, 2)
    seg, mean = numpy_merge(members, full, lo, order)
    inside = (mean > 0.5).sum(0)
    assert (inside >= 2).mean() > 0.1 and (inside == 0).mean() > 0.05
    crop = seg[1:6, 2:15, 3:20]
    assert ((crop == 3) & (mean[0] > 0.5)).any() and ((crop != 3) & (mean[0] > 0.5)).any()        # region 0 shows, and is overwritten elsewhere
    got_seg, got_mean = run(dev, members, full, lo, order=order)
    assert np.array_equal(bits(got_mean), bits(mean)) and np.array_equal(got_seg, seg)
    assert not np.array_equal(seg, numpy_merge(members, full, lo)[0])


@pytest.mark.parametrize("name", ["main", "x0_8"])
def test_everything_outside_the_crop_is_zero_and_nothing_else_is_written(dev, name):
    """the label volume lies inside a larger allocation filled with 255: the margins become 0, the guard bytes before and behind stay"""
    from cineflow import ops
    shape, full, lo = SHAPES[name]
    members, seg, _mean = case(name, 2, "fp16")
    n, guard = int(np.prod(full)), 64
    buf = torch.full((guard + n + guard,), 255, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + n].view(*full)
    ops._ensemble_merge_into([torch.from_numpy(np.array(m)).to(dev) for m in members], out, lo, None, None)
    host = buf.cpu().numpy()
    assert (host[:guard] == 255).all() and (host[guard + n:] == 255).all(), "the kernel wrote outside the label volume"
    got = host[guard:guard + n].reshape(full)
    outside = np.ones(full, dtype=bool)
    outside[tuple(slice(a, a + k) for a, k in zip(lo, shape[1:]))] = False
    assert outside.any() and not got[outside].any()
    assert np.array_equal(got, seg)


def test_grid_stride(dev):
    """626 688 eight-voxel chunks: more than the 2048 x 256 threads of the capped grid, so every thread takes the stride loop.  Uniform
    random fp16 values instead of a softmax (the kernel cannot tell), to keep the CPU side short."""
    shape, full, lo = (2, 70, 250, 250), (72, 256, 256), (1, 3, 3)
    assert full[0] * full[1] * (1 + (shape[3] + 7) // 8 + 1) > 2048 * 256
    rng = np.random.default_rng(SEED + 3)
    members = [rng.random(shape, dtype=np.float32).astype(np.float16) for _ in range(2)]
    seg, mean = numpy_merge(members, full, lo)
    got_seg, got_mean = run(dev, members, full, lo)
    assert np.array_equal(bits(got_mean), bits(mean)) and np.array_equal(got_seg, seg)


def test_ops_refusals(dev):
    from cineflow import ops
    a = torch.zeros((2, 1, 2, 3), dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="member 2 is .*float32"):
        ops.ensemble_merge([a, a, a.float()])
    with pytest.raises(ValueError, match=r"member 1 is \(2, 1, 2, 4\)"):
        ops.ensemble_merge([a, torch.zeros((2, 1, 2, 4), dtype=torch.float16, device=dev)])
    with pytest.raises(TypeError, match="member 1 must be a CUDA/HIP tensor"):
        ops.ensemble_merge([a, a.cpu()])
    with pytest.raises(ValueError, match="17 members"):
        ops.ensemble_merge([a] * 17)
    with pytest.raises(ValueError, match="do not fit"):
        ops.ensemble_merge([a], (1, 2, 4), (0, 0, 2))
    with pytest.raises(ValueError, match="regions_class_order"):
        ops.ensemble_merge([a], regions_class_order=(1, 2, 3))
    seg, mean = ops.ensemble_merge([a] * 16)                          # ENSEMBLE_MAX_MEMBERS itself is served
    assert mean is None and not seg.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ files
GEO = ((1.25, 1.5, 8.0), (10.0, -20.0, 30.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0))
CASES = ["patient001/patient001_frame00", "patient001/patient001_frame01", "patient002/patient002_frame00"]


def _props(shape, full, lo, fold):
    return {"size_after_cropping": tuple(shape), "original_size_of_raw_data": np.array(full), "crop_bbox": [[a, a + n] for a, n in zip(lo, shape)],
            "itk_spacing": GEO[0], "itk_origin": GEO[1], "itk_direction": GEO[2], "fold": fold}


def _write_folders(root, nested):
    """three seeded folders x two patients (three cases) -> (folders, {case: members})"""
    shape, full, lo = SHAPES["main"]
    folders, members = [], {c: [] for c in CASES}
    for fold in range(3):
        folder = root / ("model%d" % fold)
        folders.append(str(folder))
        for ci, c in enumerate(CASES):
            rel = c if nested else os.path.basename(c)
            path = str(folder / rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            sm = softmax_members(shape, 1, seed=100 + 10 * fold + ci)[0]
            members[c].append(sm)
            np.savez_compressed(path + ".npz", softmax=sm)
            with open(path + ".pkl", "wb") as f:
                pickle.dump(_props(shape[1:], full, lo, fold), f)
    return folders, members


@pytest.mark.parametrize("nested", [False, True], ids=["flat", "nested"])
def test_merge_writes_the_numpy_labels_with_the_input_geometry(dev, tmp_path, nested):
    from cineflow import ensemble_predictions as E
    from cineflow.nifti import read_nifti
    from cineflow.safe_pickle import load_plain_pickle
    _shape, full, lo = SHAPES["main"]
    folders, members = _write_folders(tmp_path, nested)
    out = tmp_path / "out"
    E.merge(folders, str(out), 2, store_npz=True)
    for c in CASES:
        rel = c if nested else os.path.basename(c)
        seg, mean = numpy_merge(members[c], full, lo)
        got, props = read_nifti(str(out / (rel + ".nii.gz")))
        assert got.dtype == np.uint8 and np.array_equal(got, seg)
        for key, want in zip(("itk_spacing", "itk_origin", "itk_direction"), GEO):
            assert np.allclose(props[key], want, rtol=0, atol=1e-6), key
        sm = np.load(str(out / (rel + ".npz")))["softmax"]
        assert sm.dtype == np.float16 and np.array_equal(bits(sm), bits(mean))
        plist = load_plain_pickle(str(out / (rel + ".pkl")))
        assert isinstance(plist, list) and [p["fold"] for p in plist] == [0, 1, 2]
    n_files = sum(len(f) for _d, _s, f in os.walk(str(out)))
    assert n_files == 3 * len(CASES)
    # without --npz only the label files, through merge_files as well
    out2 = tmp_path / "out2"
    E.merge(folders, str(out2), 1)
    assert sum(len(f) for _d, _s, f in os.walk(str(out2))) == len(CASES)
    rel = CASES[0] if nested else os.path.basename(CASES[0])
    one = str(tmp_path / "one.nii.gz")
    E.merge_files([os.path.join(f, rel + ".npz") for f in folders], [os.path.join(f, rel + ".pkl") for f in folders], one, True, False)
    assert np.array_equal(read_nifti(one)[0], read_nifti(str(out2 / (rel + ".nii.gz")))[0])
    assert set(E.LAST_TIMING) == {"load_s", "device_s", "write_s"} and not os.path.exists(one[:-7] + ".npz")


def test_merge_with_a_postprocessing_file(dev, tmp_path):
    from cineflow import ensemble_predictions as E
    from cineflow import predict as P
    from cineflow.nifti import read_nifti
    _shape, full, lo = SHAPES["main"]
    folders, members = _write_folders(tmp_path, True)
    pp = tmp_path / "pp_source" / "postprocessing.json"
    pp.parent.mkdir()
    pp.write_text(json.dumps({"for_which_classes": [1, 2, 3]}))
    out = tmp_path / "out"
    E.main(["-f"] + folders + ["-o", str(out), "-pp", str(pp), "-t", "2"])
    assert json.loads((out / "postprocessing.json").read_text()) == {"for_which_classes": [1, 2, 3]}
    changed = 0
    for c in CASES:
        raw, _ = read_nifti(str(out / "not_postprocessed" / (c + ".nii.gz")))
        assert np.array_equal(raw, numpy_merge(members[c], full, lo)[0])
        ref_path = str(tmp_path / "ref.nii.gz")
        P.load_remove_save(str(out / "not_postprocessed" / (c + ".nii.gz")), ref_path, [1, 2, 3], None)
        got, props = read_nifti(str(out / (c + ".nii.gz")))
        assert np.array_equal(got, read_nifti(ref_path)[0])
        assert np.allclose(props["itk_spacing"], GEO[0], rtol=0, atol=1e-6)
        changed += int((got != raw).sum())
    assert changed > 0, "the filter had nothing to remove: the check would be vacuous"


def test_two_predicted_folds_merge_to_the_numpy_statement(dev, tmp_path):
    """predict_from_folder(save_npz=True) with fold 0 and with fold 1 of a small segmentation-only model folder, then merge"""
    from cineflow import ensemble_predictions as E
    from cineflow import predict as P
    from cineflow.models import Generic_UNet
    from cineflow.nifti import read_nifti, write_nifti
    from cineflow.safe_pickle import load_plain_pickle
    from cineflow.weights import seeded_state_dict
    plans = P.default_plans(image_size=64, flow_variant=None, seg_base=8, seg_pool=3)
    seg = Generic_UNet(1, 8, 4, 3)
    model = str(tmp_path / "model")
    for fold, s in enumerate((10, 20)):
        P.save_model_folder(model, seg, None, plans, fold=fold, seg_sd=seeded_state_dict(seg.state_shapes(), s))
    inp = tmp_path / "in"
    pat, T, Z, Y, X = "patient001", 2, 2, 70, 66
    (inp / pat).mkdir(parents=True)
    g = torch.Generator().manual_seed(7)
    for t in range(T):
        vol = torch.randn(Z, Y, X, generator=g).numpy().astype(np.float32) * 40 + 100
        write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 8.0), (0, 0, 0))
    outs = [tmp_path / "out_fold0", tmp_path / "out_fold1"]
    for fold, o in enumerate(outs):
        P.predict_from_folder(model, str(inp), str(o), [fold], True, 1, 1, None, 0, 1, True)
    merged = tmp_path / "merged"
    E.merge([str(o) for o in outs], str(merged), 2)
    differ = 0
    for t in range(T):
        rel = os.path.join(pat, "%s_frame%02d" % (pat, t))
        members = [np.load(str(o / (rel + ".npz")))["softmax"] for o in outs]
        props = load_plain_pickle(str(outs[0] / (rel + ".pkl")))
        assert members[0].shape == (4, Z, Y, X) and members[0].dtype == np.float16
        lo = [int(b[0]) for b in props["crop_bbox"]] if props.get("crop_bbox") is not None else (0, 0, 0)
        want, _mean = numpy_merge(members, props["original_size_of_raw_data"] if props.get("crop_bbox") is not None else None, lo)
        got, gp = read_nifti(str(merged / (rel + ".nii.gz")))
        assert got.shape == (Z, Y, X) and np.array_equal(got, want)
        assert np.allclose(gp["itk_spacing"], (1.5, 1.5, 8.0))
        differ += int((got != read_nifti(str(outs[0] / (rel + ".nii.gz")))[0]).sum())
    assert differ > 0, "the ensemble equals fold 0 alone: the check would be vacuous"
