"""Weights trained by the reference, imported (cineflow.reference_models) and run through the HIP networks.

The fixture tree tests/golden/ref_model_folder/ holds a segmentation folder and a flow folder in the reference trainers' own layout and
the reference's outputs on seeded inputs (make_golden_refckpt.py).  Bars: the generic_unet.npz logits bar (1e-4), mean flow EPE <= 1e-4 px
(BASELINE.json north star), and for the file-level API the bound of
test_predict_api.py::test_predict_from_folder_outputs_do_not_depend_on_pool_sizes."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.join(HERE, "golden", "ref_model_folder")
S = 64


@pytest.fixture(scope="module")
def imported(tmp_path_factory):
    from cineflow import reference_models as R
    out = str(tmp_path_factory.mktemp("imported") / "model")
    R.import_reference_model_folder(os.path.join(TREE, "seg"), os.path.join(TREE, "flow"), out, crop_size=S, image_size=S)
    return out


def test_imported_networks_reproduce_the_reference_outputs(dev, imported):
    from cineflow.predict import load_model_and_checkpoint_files
    from oracle import ops as OO
    trainer, params = load_model_and_checkpoint_files(imported, [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    exp = torch.load(os.path.join(TREE, "expected_outputs.pt"), map_location="cpu", weights_only=True)
    logits = trainer.seg_net(exp["seg_x"].to(dev)).cpu()
    d = float((logits.double() - exp["seg_logits"].double()).abs().max())
    assert d <= 1e-4, "Generic_UNet logits max|diff| %.3e" % d
    flow = trainer.flow_net(exp["frames"].to(dev))["backward_flow"].cpu()
    epe = OO.mean_epe(flow, exp["backward_flow"])
    assert epe <= 1e-4, "mean EPE %.3e px" % epe


def _write_patients(inp, pats, T, Z, Y, X, seed):
    from cineflow.nifti import write_nifti
    g = torch.Generator().manual_seed(seed)
    for pat in pats:
        (inp / pat).mkdir(parents=True)
        for t in range(T):
            vol = torch.randn(Z, Y, X, generator=g).numpy().astype(np.float32) * 40 + 100
            write_nifti(str(inp / pat / ("%s_frame%02d_0000.nii.gz" % (pat, t))), vol, (1.5, 1.5, 8.0), (0, 0, 0))


def test_predict_from_folder_imported_equals_saved(dev, imported, tmp_path):
    """predict_from_folder on the imported folder and on a folder save_model_folder writes with the same weights and plans: the same files"""
    from cineflow import predict as P
    from cineflow import reference_models as R
    from cineflow.nifti import read_nifti
    with open(os.path.join(imported, "plans.json")) as f:
        plans = json.load(f)
    tr = P.CineTrainer(plans, dev, model_folder=imported)
    seg_sd = R.load_reference_checkpoint(os.path.join(TREE, "seg", "fold_0", "model_final_checkpoint.model"))["state_dict"]
    flow_sd = R.load_reference_checkpoint(os.path.join(TREE, "flow", "Task031_x", "fold_0", "model_final_checkpoint.model"))["state_dict"]
    flow_sd = {k: v for k, v in flow_sd.items() if not k.endswith("grid")}
    saved = str(tmp_path / "saved")
    P.save_model_folder(saved, tr.seg_net, tr.flow_net, plans, fold=0, seg_sd=seg_sd, flow_sd=flow_sd)
    shutil.copy(os.path.join(imported, "config.yaml"), os.path.join(saved, "config.yaml"))
    inp = tmp_path / "in"
    pats, T, Z, Y, X = ["patient001", "patient002"], 4, 2, 60, 56
    _write_patients(inp, pats, T, Z, Y, X, 21)
    outs = []
    for tag, model in (("imported", imported), ("saved", saved)):
        out = tmp_path / ("out_" + tag)
        P.predict_from_folder(model, str(inp), str(out), [0], True, 1, 2, None, 0, 1, True)
        outs.append(out)
    agree, n, dflow, dsoft = 0.0, 0, 0.0, 0.0
    for pat in pats:
        for t in range(T):
            case = "%s_frame%02d" % (pat, t)
            for sub in ("Segmentation", "Registered"):
                a, pa = read_nifti(str(outs[0] / pat / sub / (case + ".nii.gz")))
                b, pb = read_nifti(str(outs[1] / pat / sub / (case + ".nii.gz")))
                assert a.shape == b.shape == (Z, Y, X) and np.array_equal(pa["itk_spacing"], pb["itk_spacing"])
                agree += float((a == b).mean())
                n += 1
            fa, fb = np.load(str(outs[0] / pat / "Flow" / (case + ".npz"))), np.load(str(outs[1] / pat / "Flow" / (case + ".npz")))
            dflow = max(dflow, float(np.abs(fa["flow"] - fb["flow"]).max()))
            na, nb = np.load(str(outs[0] / pat / "Segmentation" / (case + ".npz"))), np.load(str(outs[1] / pat / "Segmentation" / (case + ".npz")))
            dsoft = max(dsoft, float(np.abs(na["softmax"].astype(np.float32) - nb["softmax"].astype(np.float32)).max()))
    print("imported vs saved: labels agree %.6f, flow %.1e px, softmax %.1e" % (agree / n, dflow, dsoft))
    assert agree / n >= 0.999 and dflow <= 2e-5 and dsoft <= 2e-3
