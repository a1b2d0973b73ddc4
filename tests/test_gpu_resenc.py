"""The residual-encoder U-Net (FabiansUNet3D) on the device: four BasicResidualBlock3D against the reference's blocks, the imported
fixture network against the reference's logits, and the file-level API on the imported folder.

Fixtures (make_golden_refckpt_resenc.py): tests/golden/resenc_block_<n>.npz hold input, fp32 and fp64 output of four reference
BasicResidualBlocks whose weights both sides fill from cineflow.weights (seed 300 + n); tests/golden/ref_model_folder_resenc/ is the folder
in the reference trainer's own layout with the reference's logits on a seeded input.

Bars: 2e-5 for a golden residual block against the fp64 output (the project's bar for such blocks; the reference's own fp32 drift on these
four is 2.0e-6 .. 3.0e-6, PIN_REPORT_refckpt_resenc.txt); 1e-4 for 3-D logits; bit-identical label files against exporting direct
predict_3D_3Dconv_tiled results and between pool sizes; the two-fold softmax against the mean of the single-fold runs at 2e-5.  The
generator asserts that dropping the residual branch or zeroing a projection moves these outputs by more than 1, so the bars see both."""
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RESENC = os.path.join(HERE, "golden", "ref_model_folder_resenc")
PATCH = (8, 32, 32)
PATS, T, Z, Y, X = ["patient001", "patient002"], 2, 10, 40, 36           # 2 x 2 x 2 tiles of the (8, 32, 32) patch per volume
BLOCK_SEED = 300
# (cin, cout, kernel, stride, input shape, has a projection) -- BLOCK_CASES of the generator
BLOCKS = [
    (40, 72, (3, 3, 3), (2, 2, 2), (2, 40, 5, 13, 11), True),
    (40, 72, (1, 3, 3), (1, 2, 2), (2, 40, 3, 13, 11), True),
    (72, 72, (3, 3, 3), None, (2, 72, 3, 7, 6), False),
    (72, 72, (3, 3, 3), (2, 1, 1), (2, 72, 4, 7, 6), True),
]


def _count_routes(monkeypatch):
    """counters around the strided-projection probe and the composed route, as test_gpu_unet3d_native.py counts cf_conv3d_f16s_ok"""
    from cineflow import nn as PN, ops
    asked, composed = [], []
    real_ok, real_comp = ops.conv3d_pw_f16s_ok, PN.Conv3d._forward_composed
    monkeypatch.setattr(ops, "conv3d_pw_f16s_ok", lambda *a: asked.append((a, real_ok(*a))) or asked[-1][1])
    monkeypatch.setattr(PN.Conv3d, "_forward_composed", lambda self, *a: composed.append((self.ks, self.stride)) or real_comp(self, *a))
    return asked, composed


@pytest.mark.parametrize("n", range(len(BLOCKS)))
def test_residual_block_matches_the_reference_block(dev, n, monkeypatch):
    from cineflow.nn import BasicResidualBlock3D
    from cineflow.weights import seeded_state_dict
    cin, cout, kernel, stride, shape, has_skip = BLOCKS[n]
    g = np.load(os.path.join(HERE, "golden", "resenc_block_%d.npz" % n))
    assert g["x"].shape == shape
    blk = BasicResidualBlock3D(cin, cout, kernel, stride)
    shapes = blk.state_shapes()
    assert ("downsample_skip.0.weight" in shapes) == has_skip and "downsample_skip.0.bias" not in shapes
    blk.load_state_dict(seeded_state_dict(shapes, BLOCK_SEED + n), dev)
    asked, composed = _count_routes(monkeypatch)
    x = torch.from_numpy(g["x"]).to(dev)
    x_before = x.clone()
    y = blk(x)
    torch.cuda.synchronize()
    assert torch.equal(x, x_before), "the block wrote into its input (the encoder keeps it as a skip)"
    assert len(asked) == (1 if has_skip else 0) and all(ok for _, ok in asked), asked
    assert not composed, composed
    d = float((y.cpu().double() - torch.from_numpy(g["y64"])).abs().max())
    print("\nblock %d max|diff| vs the reference in fp64: %.3e" % (n, d))
    assert d <= 2e-5, d


@pytest.mark.parametrize("n", range(len(BLOCKS)))
def test_residual_block_fp32_mode_composed_with_own_pass_norms(dev, n, monkeypatch):
    """set_conv_mode("f32"): every convolution runs composed and fuses no statistics, so each InstanceNorm3d -- the projection's one
    included, which InstanceNorm3d.forward then runs as the branch's own pass -- is a cf_group_norm call; same fp64 output, same bar"""
    from cineflow import ops
    from cineflow.nn import BasicResidualBlock3D
    from cineflow.weights import seeded_state_dict
    cin, cout, kernel, stride, shape, has_skip = BLOCKS[n]
    g = np.load(os.path.join(HERE, "golden", "resenc_block_%d.npz" % n))
    blk = BasicResidualBlock3D(cin, cout, kernel, stride)
    blk.load_state_dict(seeded_state_dict(blk.state_shapes(), BLOCK_SEED + n), dev)
    asked, composed = _count_routes(monkeypatch)
    norms = {"group_norm": 0, "group_norm_apply": 0}
    for name in norms:
        monkeypatch.setattr(ops, name, lambda *a, _real=getattr(ops, name), _name=name, **k: norms.__setitem__(_name, norms[_name] + 1) or _real(*a, **k))
    x = torch.from_numpy(g["x"]).to(dev)
    x_before = x.clone()
    ops.set_conv_mode("f32")
    try:
        y = blk(x)
    finally:
        ops.set_conv_mode("f16s")
    torch.cuda.synchronize()
    assert torch.equal(x, x_before), "the block wrote into its input (the encoder keeps it as a skip)"
    assert not asked, asked
    st = (1, 1, 1) if stride is None else stride
    assert composed == [(kernel, st), (kernel, (1, 1, 1))] + ([((1, 1, 1), st)] if has_skip else []), composed
    assert norms == {"group_norm": 3 if has_skip else 2, "group_norm_apply": 0}, norms
    d = float((y.cpu().double() - torch.from_numpy(g["y64"])).abs().max())
    print("\nblock %d in fp32 mode max|diff| vs the reference in fp64: %.3e" % (n, d))
    assert d <= 2e-5, d


@pytest.fixture(scope="module")
def imported(tmp_path_factory):
    from cineflow import reference_models as R
    out = str(tmp_path_factory.mktemp("imported_resenc") / "model")
    R.import_reference_model_folder(RESENC, None, out)
    return out


@pytest.fixture(scope="module")
def patients(tmp_path_factory):
    from cineflow.nifti import write_nifti
    inp = tmp_path_factory.mktemp("in_resenc")
    g = torch.Generator().manual_seed(31)
    for pat in PATS:
        (inp / pat).mkdir(parents=True)
        for t in range(T):
            vol = torch.randn(Z, Y, X, generator=g).numpy().astype(np.float32) * 40 + 100
            write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 10.0), (0, 0, 0))     # the stage's own spacing
    return inp


def _case_file(inp, pat, t):
    return str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t)))


def _loaded(imported, dev):
    from cineflow.predict import load_model_and_checkpoint_files
    trainer, params = load_model_and_checkpoint_files(imported, [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    return trainer


def test_imported_network_reproduces_the_reference_logits_on_the_native_projection(dev, imported, monkeypatch):
    from cineflow.models import FabiansUNet3D
    trainer = _loaded(imported, dev)
    assert isinstance(trainer.seg_net, FabiansUNet3D)
    exp = torch.load(os.path.join(RESENC, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    asked, composed = _count_routes(monkeypatch)
    logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    # the two strided projections of the fixture network: 4 -> 8 at (1,2,2) on [8,32,32], 8 -> 16 at (2,2,2) on [8,16,16]
    assert [a for a, _ in asked] == [(1, 4, 8, 32, 32, 8, (1, 2, 2)), (1, 8, 8, 16, 16, 16, (2, 2, 2))], asked
    assert all(ok for _, ok in asked)
    assert not composed, composed
    assert tuple(logits.shape) == (1, 4, 8, 32, 32)
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    d64 = float((logits.double() - exp["seg_logits_fp64"]).abs().max())
    print("\nFabiansUNet3D logits max|diff| vs the reference: %.3e (fp32), %.3e (fp64)" % (d, d64))
    assert d <= 1e-4, "FabiansUNet3D logits max|diff| %.3e" % d
    assert d64 <= 1e-4, "FabiansUNet3D logits vs fp64 max|diff| %.3e" % d64


def test_fp32_mode_runs_the_projections_composed(dev, imported, monkeypatch):
    from cineflow import ops
    trainer = _loaded(imported, dev)
    exp = torch.load(os.path.join(RESENC, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    asked, composed = _count_routes(monkeypatch)
    ops.set_conv_mode("f32")
    try:
        logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    finally:
        ops.set_conv_mode("f16s")
    assert not asked
    assert [c for c in composed if c[0] == (1, 1, 1)] == [((1, 1, 1), (1, 2, 2)), ((1, 1, 1), (2, 2, 2))], composed
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    assert d <= 1e-4, "fp32 mode max|diff| %.3e" % d


def test_predict_from_folder_equals_direct_tiled_prediction(dev, imported, patients, tmp_path):
    from cineflow import predict as P
    from cineflow.inference import predict_3D_3Dconv_tiled
    from cineflow.nifti import read_nifti
    out_a, out_b = tmp_path / "out_a", tmp_path / "out_b"
    res = P.predict_from_folder(imported, str(patients), str(out_a), [0], True, 1, 1, None, 0, 1, True)
    P.predict_from_folder(imported, str(patients), str(out_b), [0], True, 2, 2, None, 0, 1, True)
    assert sorted(res) == PATS
    trainer = _loaded(imported, dev)
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


def test_two_folds_are_the_mean_of_the_single_fold_runs(dev, imported, patients, tmp_path):
    from cineflow import predict as P
    from cineflow.models import FabiansUNet3D
    model = str(tmp_path / "model2")
    shutil.copytree(imported, model)
    ck = torch.load(os.path.join(model, "fold_0", "model_final_checkpoint.model"), map_location="cpu", weights_only=True)
    g = torch.Generator().manual_seed(5)
    ck["seg_state_dict"] = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g) for k, v in ck["seg_state_dict"].items()}
    os.makedirs(os.path.join(model, "fold_1"))
    torch.save(ck, os.path.join(model, "fold_1", "model_final_checkpoint.model"))
    trainer, params = P.load_model_and_checkpoint_files(model, None, device=dev)
    assert len(params) == 2
    d, _sg, _props = trainer.preprocess_patient([_case_file(patients, PATS[0], 0)])
    singles = []
    for p_ in params:
        trainer.load_checkpoint_ram(p_)
        singles.append(trainer.predict_preprocessed_data_return_seg_and_softmax(d)[1].astype(np.float64))
    assert float(np.abs(singles[0] - singles[1]).max()) > 1e-3, "the perturbed fold predicts the same: the check would be vacuous"
    mean = 0.5 * (singles[0] + singles[1])
    trainer.load_ensemble(params)
    assert len(trainer.seg_nets) == 2 and all(isinstance(n_, FabiansUNet3D) for n_ in trainer.seg_nets)
    seg, ens = trainer.predict_preprocessed_data_return_seg_and_softmax(d)
    err = float(np.abs(ens - mean).max())
    assert err <= 2e-5, "two-fold softmax vs the mean of the single-fold runs: %.3e" % err
    assert np.array_equal(seg, ens.argmax(0).astype(np.uint8))
