"""The cine-batched sliding window (cf_tile_gather / cf_tile_merge, inference.predict_cine_2Dconv_tiled), fold ensembles on the flow
route and on the segmentation-only route, and segmentation-only model folders through predict_from_folder.

Bars: the kernels are bit-identical to the serial crop2d / tile_accumulate / tile_finalize sequence; network outputs are held to the bars of
test_gpu_models.py::test_sliding_window_segmentation_vs_oracle (softmax max |diff| <= 5e-5, per-class Dice within 1e-3); files written by
two runs of the file-level API to the bar of test_predict_api.py::test_predict_from_folder_outputs_do_not_depend_on_pool_sizes (>= 99.9 %
of the label voxels: the floating-point atomics behind the normalisation statistics meet in another order from run to run)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.join(HERE, "golden", "ref_model_folder")
RED = dict(in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32], d_model=32, bottleneck_heads=4, dim_feedforward=48)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def load(mod, seed, dev):
    from cineflow.weights import seeded_state_dict
    mod.load_state_dict(seeded_state_dict(mod.state_shapes(), seed), dev)
    return mod


# ------------------------------------------------------------------------------------------------ kernels
# (patch, image, expected step lists): the issue's case, one tile, pw % 4 != 0 (scalar path), everything a multiple of 4 (16-byte path)
MERGE_CASES = [((64, 64), (100, 90), [[0, 18, 36], [0, 26]]),
               ((32, 48), (32, 48), [[0], [0]]),
               ((30, 22), (50, 40), None),
               ((32, 32), (48, 64), [[0, 16], [0, 16, 32]])]


@pytest.mark.parametrize("patch,image,want_steps", MERGE_CASES)
@pytest.mark.parametrize("with_gauss", [True, False])
def test_tile_merge_is_bitwise_the_serial_accumulate_finalize_sequence(dev, patch, image, want_steps, with_gauss):
    from cineflow import ops
    from cineflow.inference import compute_steps_for_sliding_window, get_gaussian
    N, K = 5, 4
    steps = compute_steps_for_sliding_window(patch, image, 0.5)
    if want_steps is not None:
        assert steps == want_steps
    tiles = [(lx, ly) for lx in steps[0] for ly in steps[1]]
    gauss = torch.from_numpy(get_gaussian(patch)).to(dev) if with_gauss else None
    pred = randn(N * len(tiles), K, patch[0], patch[1], seed=300 + len(tiles)).to(dev)
    seg, probs = ops.tile_merge(pred, gauss, image[0], image[1], steps[0], steps[1])
    assert seg.shape == (N,) + image and seg.dtype == torch.uint8 and probs.shape == (N, K) + image
    for n in range(N):
        agg = torch.zeros((K,) + image, dtype=torch.float32, device=dev)
        cnt = torch.zeros((K,) + image, dtype=torch.float32, device=dev)
        for t, (lx, ly) in enumerate(tiles):
            ops.tile_accumulate(pred[n * len(tiles) + t], gauss, agg, cnt, lx, ly)
        rseg, rprobs = ops.tile_finalize(agg, cnt)
        assert torch.equal(probs[n].view(torch.int32), rprobs.view(torch.int32)), "probs of slice %d differ bitwise" % n
        assert torch.equal(seg[n], rseg), "seg of slice %d differs" % n
    assert bool(torch.isfinite(probs).all())


@pytest.mark.parametrize("patch,image", [((64, 64), (100, 90)), ((64, 64), (100, 92)), ((30, 22), (50, 40)), ((32, 48), (32, 48))])
def test_tile_gather_is_bitwise_crop2d_for_a_shuffled_job_table(dev, patch, image):
    """image (100, 92) with a 64-wide patch takes the 16-byte path: jobs with ly % 4 == 0 load 16 bytes, the others four floats"""
    from cineflow import ops
    N, C = 5, 2
    src = randn(N, C, image[0], image[1], seed=310).to(dev)
    g = torch.Generator().manual_seed(311)
    J = 23
    n = torch.randint(0, N, (J,), generator=g)
    lx = torch.randint(0, image[0] - patch[0] + 1, (J,), generator=g)
    ly = torch.randint(0, image[1] - patch[1] + 1, (J,), generator=g)
    ly[::3] = (ly[::3] // 4) * 4
    table = torch.stack([n, lx, ly], 1)[torch.randperm(J, generator=g)].to(torch.int32)
    dst = ops.tile_gather(src, table.to(dev), patch[0], patch[1])
    assert dst.shape == (J, C) + patch
    for j in range(J):
        nj, x0, y0 = (int(v) for v in table[j])
        want = ops.crop2d(src[nj], x0, y0, patch[0], patch[1])
        assert torch.equal(dst[j].view(torch.int32), want.view(torch.int32)), j
    # a window that leaves the source reads nothing: zeros
    bad = torch.tensor([[0, image[0] - patch[0] + 1, 0], [N, 0, 0], [0, 0, -1], [1, 0, 0]], dtype=torch.int32)
    out = ops.tile_gather(src, bad.to(dev), patch[0], patch[1])
    assert float(out[:3].abs().max()) == 0.0 and torch.equal(out[3], ops.crop2d(src[1], 0, 0, patch[0], patch[1]))


# ------------------------------------------------------------------------------------------------ batched window vs oracle
def test_cine_batched_window_ensemble_vs_oracle(dev):
    """Three folds, three volumes of different in-plane shapes ((70,60) and (70,64) share the padded shape (70,64)), patch (64,64),
    4 flips, Gaussian: against the mean over the three oracle networks of the oracle's tiled prediction."""
    from cineflow.models import Generic_UNet
    from cineflow.inference import predict_cine_2Dconv_tiled, predict_3D_2Dconv_tiled
    from cineflow.weights import fill_module_
    from oracle import models as OM
    from oracle import ops as OO
    seeds = (10, 20, 30)
    nets = [load(Generic_UNet(1, 8, 4, 3), s, dev) for s in seeds]
    oras = [fill_module_(OM.GenericUNet2D(1, 8, 4, 3), s) for s in seeds]
    vols = [randn(1, 3, 100, 90, seed=98).numpy(), randn(1, 2, 70, 60, seed=97).numpy(), randn(1, 2, 70, 64, seed=96).numpy()]
    kw = dict(step_size=0.5, do_mirroring=True, mirror_axes=(0, 1), use_gaussian=True)
    got = predict_cine_2Dconv_tiled(nets, vols, (64, 64), **kw)
    assert len(got) == 3
    worst, differ = 0.0, 0.0
    for x, (seg, prob) in zip(vols, got):
        with torch.no_grad():
            per_fold = [OM.predict_3d_2dconv_tiled(o, x, (64, 64), **kw)[1] for o in oras]
        ref = np.mean(np.stack(per_fold), 0)
        rseg = ref.argmax(0)
        assert seg.shape == rseg.shape == x.shape[1:] and seg.dtype == np.uint8 and prob.shape == ref.shape
        d = float(np.abs(prob - ref).max())
        worst = max(worst, d)
        differ = max(differ, float(np.abs(ref - per_fold[0]).max()))
        print("volume %s: softmax max|diff| %.3e; ensemble vs fold 0 max %.3f, labels differing %.3f"
              % (x.shape, d, float(np.abs(ref - per_fold[0]).max()), float((rseg != per_fold[0].argmax(0)).mean())))
        assert d <= 5e-5, d
        for k in range(4):
            dc = OO.dice(seg, rseg, k)
            assert np.isnan(dc) or abs(dc - 1.0) <= 1e-3, (k, dc)
    assert differ > 0.1, "the ensemble must differ from fold 0, or a fold-0-only implementation would pass"
    # one network, one volume: predict_3D_2Dconv_tiled's own result (the same tiles through the same kernels, merged in gather form)
    seg1, prob1 = predict_cine_2Dconv_tiled(nets[0], [vols[0]], (64, 64), **kw)[0]
    seg0, prob0 = predict_3D_2Dconv_tiled(nets[0], vols[0], (64, 64), **kw)
    assert float(np.abs(prob1 - prob0).max()) <= 5e-5 and float((seg1 == seg0).mean()) >= 0.999
    # chunks that cut through a slice's tiles give the same result as one chunk per group
    segc, probc = predict_cine_2Dconv_tiled(nets[:2], vols[1:], (64, 64), max_batch=3, **kw)[1]
    segw, probw = predict_cine_2Dconv_tiled(nets[:2], vols[1:], (64, 64), max_batch=1000, **kw)[1]
    assert float(np.abs(probc - probw).max()) <= 5e-5


# ------------------------------------------------------------------------------------------------ flow route
def _two_fold_flow_folder(folder):
    from cineflow import predict as P
    from cineflow.models import SegFlowGaussian, Generic_UNet
    from cineflow.weights import seeded_state_dict
    plans = P.default_plans(image_size=64, crop_size=64, flow_variant="video", seg_base=8, seg_pool=3, reduced=RED)
    seg = Generic_UNet(1, 8, 4, 3)
    flow = SegFlowGaussian(image_size=64, motion_appearance=False, **RED)
    for fold, (ss, fs) in enumerate(((10, 11), (20, 21))):
        sd_s = seeded_state_dict({k: v for k, v in seg.state_shapes().items()}, ss)
        sd_f = seeded_state_dict({k: v for k, v in flow.state_shapes().items() if not k.endswith("grid")}, fs)
        P.save_model_folder(folder, seg, flow, plans, fold=fold, seg_sd=sd_s, flow_sd=sd_f)


def _write_patients(inp, pats, T, Z, Y, X, seed):
    from cineflow.nifti import write_nifti
    g = torch.Generator().manual_seed(seed)
    for pat in pats:
        (inp / pat).mkdir(parents=True)
        for t in range(T):
            vol = torch.randn(Z, Y, X, generator=g).numpy().astype(np.float32) * 40 + 100
            write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 8.0), (0, 0, 0))


def _label_agreement(o1, o2, pats, T, subs):
    from cineflow.nifti import read_nifti
    agree, n = 0.0, 0
    for pat in pats:
        for t in range(T):
            for sub in subs:
                name = "%s_frame%02d.nii.gz" % (pat, t)
                a, _ = read_nifti(os.path.join(str(o1), pat, sub, name))
                b, _ = read_nifti(os.path.join(str(o2), pat, sub, name))
                assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
                agree += float((a == b).mean())
                n += 1
    return agree / n


def test_flow_route_ensembles_the_softmax_and_keeps_fold_0_flow(dev, tmp_path):
    from cineflow import ops
    from cineflow import predict as P
    from oracle import ops as OO
    model = str(tmp_path / "model")
    _two_fold_flow_folder(model)
    T, Z = 4, 2
    unl = (randn(T, 1, Z, 64, 64, seed=16) * 30 + 80).numpy().astype(np.float32)
    runs = {}
    for folds in ([0, 1], [0], [1]):
        trainer, params = P.load_model_and_checkpoint_files(model, folds, device=dev)
        assert len(params) == len(folds)
        trainer.load_ensemble(params)
        assert len(trainer.seg_nets) == len(folds)
        runs[tuple(folds)] = trainer.predict_preprocessed_data_return_seg_and_softmax_flow(unl)[:4]
    seg, soft, flow, reg = runs[(0, 1)]
    _s0, soft0, flow0, _r0 = runs[(0,)]
    _s1, soft1, flow1, _r1 = runs[(1,)]
    d = float(np.abs(soft - (soft0.astype(np.float64) + soft1) / 2).max())
    apart = float(np.abs(soft0 - soft1).max())
    epe = OO.mean_epe(torch.from_numpy(flow), torch.from_numpy(flow0))
    epe_other = OO.mean_epe(torch.from_numpy(flow), torch.from_numpy(flow1))
    print("ensemble vs mean of single folds %.3e; folds apart %.3f; flow vs fold 0 %.3e px, vs fold 1 %.3e px" % (d, apart, epe, epe_other))
    assert d <= 5e-5, d
    assert apart > 0.1, apart
    assert epe <= 2e-5, epe                                                       # the flow is the first selected fold's
    assert epe_other > 1e-2, epe_other                                            # ... and not the other fold's, nor an average
    ed = soft[0].argmax(0).astype(np.uint8)                                       # [Z,Y,X]: arg-max of the ENSEMBLED ED softmax
    assert np.array_equal(seg[0], ed)
    assert np.array_equal(reg[0, 0], ed), "the registered ED frame is the ensembled ED arg-max"
    assert float((ed != soft0[0].argmax(0)).mean()) > 0.01                        # which is not fold 0's arg-max
    flow_dev = torch.from_numpy(np.ascontiguousarray(flow.transpose(0, 2, 1, 3, 4))).to(dev)      # [T,Z,2,Y,X]
    want = ops.warp_labels(flow_dev, torch.from_numpy(ed).to(dev)).cpu().numpy()
    agree = float((reg[:, 0] == want).mean())
    assert agree >= 0.999, agree


def test_predict_from_folder_folds_none_takes_every_fold(dev, tmp_path):
    """folds=None finds fold_0 and fold_1: the label files are those of folds=[0, 1], not those of fold 0 alone"""
    from cineflow import predict as P
    model = str(tmp_path / "model")
    _two_fold_flow_folder(model)
    inp = tmp_path / "in"
    pats, T = ["patient001", "patient002"], 4
    _write_patients(inp, pats, T, 2, 60, 56, 5)
    outs = {}
    for tag, folds in (("none", None), ("both", [0, 1]), ("zero", [0])):
        outs[tag] = tmp_path / ("out_" + tag)
        P.predict_from_folder(model, str(inp), str(outs[tag]), folds, False, 2, 2, None, 0, 1, True)
    same = _label_agreement(outs["none"], outs["both"], pats, T, ("Segmentation", "Registered"))
    other = _label_agreement(outs["none"], outs["zero"], pats, T, ("Segmentation", "Registered"))
    print("folds=None vs [0,1]: labels agree %.6f; vs [0]: %.6f" % (same, other))
    assert same >= 0.999, same
    assert other < 0.99, other


# ------------------------------------------------------------------------------------------------ segmentation-only folder
def test_predict_from_folder_segmentation_only(dev, tmp_path):
    from cineflow import predict as P
    from cineflow.models import Generic_UNet
    from cineflow.nifti import read_nifti
    from cineflow.weights import seeded_state_dict, fill_module_
    from oracle import models as OM
    from oracle import ops as OO
    plans = P.default_plans(image_size=64, flow_variant=None, seg_base=8, seg_pool=3)
    seg = Generic_UNet(1, 8, 4, 3)
    model = str(tmp_path / "model")
    seeds = (10, 20)
    for fold, s in enumerate(seeds):
        P.save_model_folder(model, seg, None, plans, fold=fold, seg_sd=seeded_state_dict(seg.state_shapes(), s))
    inp = tmp_path / "in"
    pats, T, Z, Y, X = ["patient001", "patient002"], 4, 2, 90, 70        # larger than the (64, 64) patch: 2 x 2 tiles per slice
    _write_patients(inp, pats, T, Z, Y, X, 7)
    with open(str(inp / "patient002" / "patient002.csv"), "w") as f:   # an ED index must change nothing on this route
        f.write("ed_index,es_index\n1,3\n")
    out = tmp_path / "out_a"
    res = P.predict_from_folder(model, str(inp), str(out), None, True, 1, 1, None, 0, 1, True)
    assert sorted(res) == pats
    assert P.LAST_TIMING["patients"] == 2 and P.LAST_TIMING["frames"] == 2 * T and P.LAST_TIMING["device_batches"] >= 1 and P.LAST_TIMING["total_s"] > 0
    oras = [fill_module_(OM.GenericUNet2D(1, 8, 4, 3), s) for s in seeds]
    trainer, _ = P.load_model_and_checkpoint_files(model, None, device=dev)
    agree, n = 0.0, 0
    for pat in pats:
        assert sorted(os.listdir(str(out / pat))) == sorted("%s_frame%02d%s" % (pat, t, e) for t in range(T) for e in (".nii.gz", ".npz", ".pkl"))
        assert res[pat] == [str(out / pat / ("%s_frame%02d.nii.gz" % (pat, t))) for t in range(T)]
        for t in range(T):
            case = "%s_frame%02d" % (pat, t)
            s, pr = read_nifti(str(out / pat / (case + ".nii.gz")))
            assert s.shape == (Z, Y, X) and s.dtype == np.uint8 and s.max() <= 3 and np.allclose(pr["itk_spacing"], (1.5, 1.5, 8.0))
            sm = np.load(str(out / pat / (case + ".npz")))["softmax"]
            assert sm.shape == (4, Z, Y, X) and sm.dtype == np.float16
            # values: the export of the oracle's tiled softmax (mean over the folds) of the same preprocessed frame
            d, _sg, props = trainer.preprocess_patient([str(inp / pat / (case + "_0000.nii.gz"))])
            with torch.no_grad():
                ref = np.mean(np.stack([OM.predict_3d_2dconv_tiled(o, d, (64, 64), step_size=0.5, do_mirroring=True, mirror_axes=(0, 1),
                                                                   use_gaussian=True)[1] for o in oras]), 0)
            ref_path = str(tmp_path / ("ref_" + case + ".nii.gz"))
            P.save_segmentation_nifti_from_softmax(ref.astype(np.float32), ref_path, props, 1, None, None, None, None, None, None, 0, False)
            r, _ = read_nifti(ref_path)
            agree += float((s == r).mean())
            n += 1
    print("segmentation-only export vs export of the oracle's tiled softmax: labels agree %.6f" % (agree / n))
    assert agree / n >= 0.999
    # pool sizes only change when things happen
    out_b = tmp_path / "out_b"
    P.predict_from_folder(model, str(inp), str(out_b), None, True, 4, 4, None, 0, 1, True)
    same = _label_agreement(out, out_b, pats, T, ("",))
    print("pool sizes (1,1) vs (4,4): labels agree %.6f" % same)
    assert same >= 0.999
    for o in (out, out_b):
        for pat in pats:
            assert not os.path.exists(str(o / pat / "Flow")) and not os.path.exists(str(o / pat / "Registered")) and not os.path.exists(str(o / pat / "Segmentation"))
    # sharding as on the flow route, and without save_npz only the label files
    res1 = P.predict_from_folder(model, str(inp), str(tmp_path / "out1"), None, False, 1, 1, None, 1, 2, False)
    assert sorted(res1) == ["patient002"]
    assert sorted(os.listdir(str(tmp_path / "out1" / "patient002"))) == ["patient002_frame%02d.nii.gz" % t for t in range(T)]
    # postprocessing.json (predict.py:1139-1156): only the largest component of each class survives
    with open(os.path.join(model, "postprocessing.json"), "w") as f:
        json.dump({"for_which_classes": [1, 2, 3]}, f)
    P.predict_from_folder(model, str(inp), str(tmp_path / "out2"), None, False, 1, 1, None, 1, 2, False)
    assert os.path.isfile(str(tmp_path / "out2" / "patient002" / "postprocessing.json"))
    changed = 0
    for t in range(T):
        case = "patient002_frame%02d.nii.gz" % t
        raw, _ = read_nifti(str(tmp_path / "out1" / "patient002" / case))
        pp, _ = read_nifti(str(tmp_path / "out2" / "patient002" / case))
        ref = OO.remove_all_but_the_largest_connected_component(raw.copy(), [1, 2, 3], 1.5 * 1.5 * 8.0, None)[0]
        if float((pp == ref).mean()) < 1.0:
            # the two runs' raw labels may differ in a few near-tie voxels: then compare with the filter applied to this run's own input
            assert float((pp == ref).mean()) >= 0.99
        changed += int((ref != raw).sum())
    assert changed > 0, "the filter had nothing to remove: the check would be vacuous"
    # predict_cases on one patient: the same route
    lol = [[str(inp / "patient001" / ("patient001_frame%02d_0000.nii.gz" % t))] for t in range(T)]
    outs = [str(tmp_path / "out3" / "patient001" / ("patient001_frame%02d.nii.gz" % t)) for t in range(T)]
    got = P.predict_cases(model, lol, outs, None, False, 1, 1, disable_postprocessing=True)
    assert got == outs and all(os.path.isfile(o) for o in outs)


# ------------------------------------------------------------------------------------------------ reference-written folder
def test_reference_written_segmentation_folder_on_its_own(dev, tmp_path):
    from cineflow import predict as P
    from cineflow import reference_models as R
    from cineflow.nifti import read_nifti
    out = str(tmp_path / "model")
    R.import_reference_model_folder(os.path.join(TREE, "seg"), None, out)
    trainer, params = P.load_model_and_checkpoint_files(out, None, device=dev)
    trainer.load_checkpoint_ram(params[0])
    exp = torch.load(os.path.join(TREE, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    assert d <= 1e-4, "Generic_UNet logits max|diff| %.3e" % d
    inp = tmp_path / "in"
    pats, T, Z, Y, X = ["patient001"], 3, 2, 60, 56
    _write_patients(inp, pats, T, Z, Y, X, 21)
    res = P.predict_from_folder(out, str(inp), str(tmp_path / "out"), None, False, 1, 1, None, 0, 1, True)
    assert len(res["patient001"]) == T
    for pth in res["patient001"]:
        s, _ = read_nifti(pth)
        assert s.shape == (Z, Y, X) and s.dtype == np.uint8 and s.max() <= 3
