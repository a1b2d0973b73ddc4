"""A `3d_fullres` folder trained by the reference, imported (cineflow.reference_models) and served by the file-level API on the native 3-D
convolution.  The fixture tree tests/golden/ref_model_folder_3d/ holds the folder in the reference trainer's own layout and the reference's
logits on a seeded input (make_golden_refckpt3d.py).

Bars: the generic_unet_3d.npz logits bar (1e-4); bit-identical label files against exporting direct predict_3D_3Dconv_tiled results, and
between pool sizes; the two-fold softmax against the mean of the two single-fold runs at 2e-5 in fp32 (the tiled-softmax bar).  The `.npz`
file stores the softmax as float16 (save_segmentation_nifti_from_softmax), so the file is held to the same mean at 2e-5 plus fp16's
rounding of the stored value, u |p| with fp16's unit roundoff u = 2^-11 -- the fp32 comparison next to it carries the 2e-5 alone."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEG3D = os.path.join(HERE, "golden", "ref_model_folder_3d")
PATCH = (8, 32, 32)
PATS, T, Z, Y, X = ["patient001", "patient002"], 2, 10, 40, 36           # 2 x 2 x 2 tiles of the (8, 32, 32) patch per volume


@pytest.fixture(scope="module")
def imported(tmp_path_factory):
    from cineflow import reference_models as R
    out = str(tmp_path_factory.mktemp("imported3d") / "model")
    R.import_reference_model_folder(SEG3D, None, out)
    return out


@pytest.fixture(scope="module")
def patients(tmp_path_factory):
    from cineflow.nifti import write_nifti
    inp = tmp_path_factory.mktemp("in3d")
    g = torch.Generator().manual_seed(31)
    for pat in PATS:
        (inp / pat).mkdir(parents=True)
        for t in range(T):
            vol = torch.randn(Z, Y, X, generator=g).numpy().astype(np.float32) * 40 + 100
            write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 10.0), (0, 0, 0))     # the stage's own spacing
    return inp


def _case_file(inp, pat, t):
    return str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t)))


def test_imported_3d_network_reproduces_the_reference_logits(dev, imported):
    from cineflow.models import Generic_UNet3D
    from cineflow.predict import load_model_and_checkpoint_files
    trainer, params = load_model_and_checkpoint_files(imported, [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    assert isinstance(trainer.seg_net, Generic_UNet3D)
    exp = torch.load(os.path.join(SEG3D, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    assert d <= 1e-4, "Generic_UNet3D logits max|diff| %.3e" % d


def test_predict_from_folder_3d_equals_direct_tiled_prediction(dev, imported, patients, tmp_path):
    from cineflow import predict as P
    from cineflow.inference import predict_3D_3Dconv_tiled
    from cineflow.nifti import read_nifti
    out_a, out_b = tmp_path / "out_a", tmp_path / "out_b"
    res = P.predict_from_folder(imported, str(patients), str(out_a), [0], True, 1, 1, None, 0, 1, True)
    P.predict_from_folder(imported, str(patients), str(out_b), [0], True, 2, 2, None, 0, 1, True)
    assert sorted(res) == PATS
    trainer, params = P.load_model_and_checkpoint_files(imported, [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    for pat in PATS:
        assert sorted(os.listdir(str(out_a / pat))) == sorted("%s_frame%02d%s" % (pat, t, e) for t in range(T) for e in (".nii.gz", ".npz", ".pkl"))
        assert res[pat] == [str(out_a / pat / ("%s_frame%02d.nii.gz" % (pat, t))) for t in range(T)]
        for t in range(T):
            case = "%s_frame%02d" % (pat, t)
            s, pr = read_nifti(str(out_a / pat / (case + ".nii.gz")))
            assert s.shape == (Z, Y, X) and s.dtype == np.uint8 and s.max() <= 3 and np.allclose(pr["itk_spacing"], (1.5, 1.5, 10.0))
            d, _sg, props = trainer.preprocess_patient([_case_file(patients, pat, t)])
            assert d.shape == (1, Z, Y, X)
            _seg, prob = predict_3D_3Dconv_tiled(trainer.seg_net, d, PATCH, 0.5, True, (0, 1, 2), True)
            ref_path = str(tmp_path / ("ref_" + case + ".nii.gz"))
            P.save_segmentation_nifti_from_softmax(prob, ref_path, props, 1, None, None, None, None, None, None, 0, False)
            r, _ = read_nifti(ref_path)
            assert np.array_equal(s, r), "%s: %d voxels differ from the export of the direct tiled prediction" % (case, int((s != r).sum()))
            sb, _ = read_nifti(str(out_b / pat / (case + ".nii.gz")))
            assert np.array_equal(s, sb), "%s: the labels depend on the pool sizes" % case
            sm = np.load(str(out_a / pat / (case + ".npz")))["softmax"]
            assert sm.shape == (4, Z, Y, X) and sm.dtype == np.float16
        assert not os.path.exists(str(out_a / pat / "Segmentation")) and not os.path.exists(str(out_a / pat / "Flow"))


def test_two_folds_are_the_mean_of_the_single_fold_runs(dev, imported, patients, tmp_path):
    from cineflow import predict as P
    model = str(tmp_path / "model2")
    shutil.copytree(imported, model)
    ck = torch.load(os.path.join(model, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    g = torch.Generator().manual_seed(5)
    ck["seg_state_dict"] = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g) for k, v in ck["seg_state_dict"].items()}
    os.makedirs(os.path.join(model, "fold_1"))
    torch.save(ck, os.path.join(model, "fold_1", "model_final_checkpoint.model"))
    trainer, params = P.load_model_and_checkpoint_files(model, None, device=dev)
    assert len(params) == 2
    pat = PATS[0]
    inp1 = tmp_path / "in1"
    shutil.copytree(str(patients / pat), str(inp1 / pat))
    P.predict_from_folder(model, str(inp1), str(tmp_path / "out"), None, True, 1, 1, None, 0, 1, True)
    for t in range(T):
        d, _sg, _props = trainer.preprocess_patient([_case_file(patients, pat, t)])
        singles = []
        for p_ in params:
            trainer.load_checkpoint_ram(p_)
            singles.append(trainer.predict_preprocessed_data_return_seg_and_softmax(d)[1].astype(np.float64))
        assert float(np.abs(singles[0] - singles[1]).max()) > 1e-3, "the perturbed fold predicts the same: the check would be vacuous"
        mean = 0.5 * (singles[0] + singles[1])
        trainer.load_ensemble(params)
        seg, ens = trainer.predict_preprocessed_data_return_seg_and_softmax(d)
        err = float(np.abs(ens - mean).max())
        assert err <= 2e-5, "two-fold softmax vs the mean of the single-fold runs: %.3e" % err
        assert np.array_equal(seg, ens.argmax(0).astype(np.uint8))
        sm = np.load(str(tmp_path / "out" / pat / ("%s_frame%02d.npz" % (pat, t))))["softmax"]
        assert sm.dtype == np.float16 and sm.shape == mean.shape
        excess = float((np.abs(sm.astype(np.float64) - mean) - 2.0 ** -11 * np.abs(mean)).max())
        assert excess <= 2e-5, "the .npz softmax vs the mean of the single-fold runs, beyond fp16 storage: %.3e" % excess
