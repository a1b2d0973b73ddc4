"""A `3d_cascade_fullres` folder trained by the reference, imported (cineflow.reference_models) and served by the file-level API with the
previous stage's labels as input channels.  The fixture tree tests/golden/ref_model_folder_cascade/ holds both stages' folders in the
reference trainer's own layout, the reference network's logits on a seeded 4-channel input and what the reference's preprocess_save
returns for a seeded label map (make_golden_refckpt_cascade.py).

Input: 2 patients x 2 frames of (10, 40, 36) volumes at the full-resolution stage's spacing, zero outside [:, 4:36, 2:34], so the crop to
non-zero leaves a (10, 32, 32) grid.  The previous stage's label file is UNCROPPED (10, 40, 36) and is resized onto that grid as the
reference does it: ratios 1, 40/32 = 1.25 and 36/32 = 1.125, so every per-axis weight is a multiple of 1/8 or 1/16 and every product and
sum is exact in fp32 and in float64, in any order.  That is why the network input can be held to the oracle bit for bit whatever
labels the lowres network happens to predict (indicators of exactly 0.5 included) by any arithmetic; ties whose weights round are
held to the oracle by tests/test_gpu_label_resize.py.

Bars: the generic_unet_3d.npz logits bar (1e-4, as test_gpu_reference_import_3d.py); the exported fp16 softmax against the direct route
at 2^-10 (one fp16 ulp below 1.0 is 2^-11, doubled for values that straddle a rounding boundary); label files equal wherever the
direct route's top-two margin is >= 2^-9, and at most 1 % of the volume may lie below that margin."""
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASCADE = os.path.join(HERE, "golden", "ref_model_folder_cascade")
PATCH = (8, 32, 32)
PATS, T, Z, Y, X = ["patient001", "patient002"], 2, 10, 40, 36
BOX = (slice(None), slice(4, 36), slice(2, 34))                          # the non-zero part of every volume
CLASSES = [1, 2, 3]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from cineflow import reference_models as R
    root = tmp_path_factory.mktemp("imported_cascade")
    full, low = str(root / "cascade"), str(root / "lowres")
    R.import_reference_model_folder(CASCADE, None, full)
    R.import_reference_model_folder(os.path.join(CASCADE, "lowres"), None, low)
    return full, low


@pytest.fixture(scope="module")
def patients(tmp_path_factory):
    from cineflow.nifti import write_nifti
    inp = tmp_path_factory.mktemp("in_cascade")
    g = torch.Generator().manual_seed(41)
    for pat in PATS:
        (inp / pat).mkdir(parents=True)
        for t in range(T):
            vol = np.zeros((Z, Y, X), np.float32)
            vol[BOX] = torch.randn(Z, 32, 32, generator=g).numpy() * 40 + 100
            write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 10.0), (0, 0, 0))
    return inp


@pytest.fixture(scope="module")
def two_step(dev, models, patients, tmp_path_factory):
    """the lowres run, then the cascade run on its output folder as it is: (lowres_out, out, returned paths)"""
    from cineflow import predict as P
    root = tmp_path_factory.mktemp("out_cascade")
    lowres_out, out = root / "lowres_out", root / "out"
    P.predict_from_folder(models[1], str(patients), str(lowres_out), [0], False, 1, 1, None, 0, 1, True)
    res = P.predict_from_folder(models[0], str(patients), str(out), [0], True, 2, 2, str(lowres_out), 0, 1, True)
    return lowres_out, out, res


def _case_file(inp, pat, t):
    return str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t)))


def _trainer(model, dev):
    from cineflow.predict import load_model_and_checkpoint_files
    trainer, params = load_model_and_checkpoint_files(model, [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    return trainer


def test_imported_cascade_network_reproduces_the_reference_logits(dev, models):
    from cineflow.models import Generic_UNet3D
    trainer = _trainer(models[0], dev)
    assert isinstance(trainer.seg_net, Generic_UNet3D) and trainer.seg_net.input_channels == 4 and trainer.prev_stage_classes == CLASSES
    exp = torch.load(os.path.join(CASCADE, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    assert tuple(exp["seg_x"].shape) == (1, 4) + PATCH
    logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    print("cascade Generic_UNet3D logits max|diff| %.3e" % d)
    assert d <= 1e-4, "Generic_UNet3D logits max|diff| %.3e" % d


def test_prev_stage_to_input_reproduces_the_reference_preprocess_save(dev):
    from cineflow import preprocessing as P
    exp = torch.load(os.path.join(CASCADE, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    data, seg = exp["prev_data"].numpy(), exp["prev_seg"].numpy()
    assert tuple(exp["prev_target_shape"].tolist()) == data.shape[1:] and seg.shape != data.shape[1:]
    got = P.prev_stage_to_input(data, seg, CLASSES)
    want = exp["prev_input"].numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want), "%d values differ from the reference's preprocess_save" % int((got != want).sum())


def test_cascade_run_consumes_the_lowres_output_folder(dev, models, patients, two_step, tmp_path):
    from cineflow import predict as P
    from cineflow.inference import predict_3D_3Dconv_tiled
    from cineflow.nifti import read_nifti
    from oracle import preprocess as OP
    lowres_out, out, res = two_step
    assert sorted(res) == PATS
    trainer = _trainer(models[0], dev)
    plain_plans = dict(trainer.plans, seg_net={k: v for k, v in trainer.plans["seg_net"].items() if k != "prev_stage_classes"})
    plain = P.CineTrainer(plain_plans, dev)                                  # the same preprocessing without the label channels
    below, total = 0, 0
    for pat in PATS:
        assert res[pat] == [str(out / pat / ("%s_frame%02d.nii.gz" % (pat, t))) for t in range(T)]
        for t in range(T):
            case = "%s_frame%02d" % (pat, t)
            files, low_file = [_case_file(patients, pat, t)], str(lowres_out / pat / (case + ".nii.gz"))
            seg_prev, _ = read_nifti(low_file)
            assert seg_prev.shape == (Z, Y, X) and seg_prev.max() <= 3
            d0 = plain.preprocess_patient(files)[0]
            assert d0.shape == (1, Z, 32, 32)
            resized = OP.resize_segmentation(seg_prev.transpose(trainer.plans["transpose_forward"]), d0.shape[1:], order=1)
            onehot = np.stack([(resized == c) for c in CLASSES]).astype(np.float32)
            want = np.vstack((d0, onehot)).astype(np.float32)
            x, _sg, props = trainer.preprocess_patient(files, seg_from_prev_stage=low_file)
            assert x.dtype == np.float32 and x.shape == (4, Z, 32, 32)
            assert np.array_equal(x, want), "%s: %d network-input values differ from vstack(data, oracle one-hot)" % (case, int((x != want).sum()))
            # the direct route on that input, exported by the same function
            _seg, prob = predict_3D_3Dconv_tiled(trainer.seg_net, x, PATCH, 0.5, True, (0, 1, 2), True)
            ref_path = str(tmp_path / ("ref_" + case + ".nii.gz"))
            P.save_segmentation_nifti_from_softmax(prob, ref_path, props, 1, None, None, None, ref_path[:-7] + ".npz", None, None, 0, False)
            sm = np.load(str(out / pat / (case + ".npz")))["softmax"]
            sm_ref = np.load(ref_path[:-7] + ".npz")["softmax"]
            assert sm.dtype == np.float16 and sm.shape == (4, Z, 32, 32) == sm_ref.shape
            err = float(np.abs(sm.astype(np.float64) - sm_ref.astype(np.float64)).max())
            assert err <= 2.0 ** -10, "%s: exported softmax vs the direct route: %.3e" % (case, err)
            s, pr = read_nifti(str(out / pat / (case + ".nii.gz")))
            r, _ = read_nifti(ref_path)
            assert s.shape == (Z, Y, X) and s.dtype == np.uint8 and np.allclose(pr["itk_spacing"], (1.5, 1.5, 10.0))
            top2 = np.sort(prob.astype(np.float64), axis=0)[-2:]
            sure = np.zeros((Z, Y, X), bool)
            sure[BOX] = (top2[1] - top2[0]) >= 2.0 ** -9
            outside = np.ones((Z, Y, X), bool)
            outside[BOX] = False
            assert not s[outside].any() and not r[outside].any()
            assert np.array_equal(s[sure], r[sure]), "%s: %d decided voxels differ from the direct route" % (case, int((s[sure] != r[sure]).sum()))
            below += int((~sure[BOX]).sum())
            total += sure[BOX].size
    print("voxels below the 2^-9 margin: %d of %d (%.4f)" % (below, total, below / total))
    assert below <= 0.01 * total, "%.4f of the volume lies below the top-two margin 2^-9 (cap 1 %%)" % (below / total)


def test_all_zero_previous_stage_labels_change_the_output(dev, models, patients, two_step, tmp_path):
    """the label channels are consumed: the same patient with an all-background previous stage predicts something else"""
    from cineflow import predict as P
    from cineflow.nifti import write_nifti
    _lowres_out, out, _res = two_step
    pat = PATS[0]
    inp1, zeros = tmp_path / "in1", tmp_path / "zeros"
    shutil.copytree(str(patients / pat), str(inp1 / pat))
    zeros.mkdir()
    for t in range(T):                                                       # the reference's flat layout: <l>/<case>.nii.gz
        write_nifti(str(zeros / ("%s_frame%02d.nii.gz" % (pat, t))), np.zeros((Z, Y, X), np.uint8), (1.5, 1.5, 10.0), (0, 0, 0))
    P.predict_from_folder(models[0], str(inp1), str(tmp_path / "out0"), [0], True, 1, 1, str(zeros), 0, 1, True)
    for t in range(T):
        case = "%s_frame%02d" % (pat, t)
        a = np.load(str(out / pat / (case + ".npz")))["softmax"].astype(np.float64)
        b = np.load(str(tmp_path / "out0" / pat / (case + ".npz")))["softmax"].astype(np.float64)
        assert float(np.abs(a - b).max()) > 1e-2, "%s: the previous stage's labels do not reach the network" % case


def test_lowres_model_flag_gives_the_files_of_the_two_step_run(dev, models, patients, two_step, tmp_path):
    from cineflow import predict as P
    from cineflow.nifti import read_nifti
    lowres_out, out, _res = two_step
    out2 = tmp_path / "out2"
    P.main(["-i", str(patients), "-o", str(out2), "-m", models[0], "--lowres_model", models[1], "-f", "0",
            "--num_threads_preprocessing", "2", "--num_threads_nifti_save", "2"])
    for pat in PATS:
        for t in range(T):
            case = "%s_frame%02d.nii.gz" % (pat, t)
            assert np.array_equal(read_nifti(str(out2 / "3d_lowres_predictions" / pat / case))[0], read_nifti(str(lowres_out / pat / case))[0])
            assert np.array_equal(read_nifti(str(out2 / pat / case))[0], read_nifti(str(out / pat / case))[0]), case


def test_model_folder_and_lowres_folder_mismatches_raise(dev, models, patients, two_step, tmp_path):
    from cineflow import predict as P
    lowres_out, _out, _res = two_step
    with pytest.raises(ValueError, match="-l"):
        P.predict_from_folder(models[0], str(patients), str(tmp_path / "a"), [0], False, 1, 1, None, 0, 1, True)
    with pytest.raises(ValueError, match="lowres"):                          # (the message names the model folder, here .../lowres)
        P.predict_from_folder(models[1], str(patients), str(tmp_path / "b"), [0], False, 1, 1, str(lowres_out), 0, 1, True)
    trainer = _trainer(models[0], dev)
    with pytest.raises(ValueError, match="-l"):
        trainer.preprocess_patient([_case_file(patients, PATS[0], 0)])
    with pytest.raises(ValueError, match="-l"):
        P.predict_cases(models[0], [[_case_file(patients, PATS[0], 0)]], [str(tmp_path / "c" / "x.nii.gz")], [0], False, 1, 1)


@pytest.mark.parametrize("k", [(1, 3, 3), (3, 3, 3)], ids=["k133", "k333"])
def test_conv3d_f16s_serves_the_first_layer_at_four_input_channels(dev, k):
    """the cascade's first convolution, Conv3d(1 + 3, 4, k) at the fixture's patch: the native kernel takes it (no fallback) and holds the
    split-exact bar of test_gpu_conv3d_routes.py (|out - y3| <= 2^-18 A), which a dropped last input channel -- the third label plane --
    would miss"""
    from _split_exact import SPLIT_BAR, randn, ratio
    from cineflow import ops
    from test_gpu_conv3d_routes import split_reference
    B, C, Cout, (D, H, W), st = 1, 4, 4, PATCH, (1, 1, 1)
    x = randn(B, C, D, H, W, seed=4000 + k[0])
    x[:, 1:] = (x[:, 1:] > 0.5).float()                                      # label planes hold zeros and ones
    w = randn(Cout, C, *k, seed=4010 + k[0]) / (C * k[0] * 9) ** 0.5
    b = randn(Cout, seed=4020 + k[0])
    assert ops.conv3d_f16s_ok(B, C, 0, D, H, W, Cout, k, st), "the probe declines the cascade's first layer: a fallback would be serving it"
    wpk, s = ops.pack_conv3d_weight_f16s(w.to(dev))
    ref = split_reference(x, w, b, s, lambda a, m: F.conv3d(a, m, stride=st, padding=(k[0] // 2, 1, 1)))
    out, _ws = ops.conv3d_f16s(x.to(dev), wpk, s, b.to(dev), Cout, k, st, stats_groups=Cout)
    o = out.cpu().double()
    bar = SPLIT_BAR * ref["A"]
    worst = ratio(o, ref["y3"], bar)
    print("first layer C1 = 4, k = %s: worst |out - y3| / (2^-18 A) = %.4f" % (k, worst))
    assert worst <= 1.0, ("split-exact", worst)
    assert ratio(o, ref["y3"] - ref["d3"], bar) > 1.0, "a dropped last input channel would pass the bar"
    assert float((o - ref["true"]).abs().max()) <= 1e-5
