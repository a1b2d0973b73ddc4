"""Model folders of the reference's architectural trainer variants (tests/golden/ref_model_variants, make_golden_variants.py), imported
with cineflow.reference_models and run on the HIP networks, 2-D and 3-D.

Logits: the bar tests/test_gpu_models.py applies to the reduced-width Generic_UNet / generic_unet_3d fixtures (1e-4), against the logits
the reference's own network gave on the CPU.  Labels: identical wherever the reference's top two logits differ by more than that bar; the
share of voxels inside it is at most 1 % (0.34 % at the worst, nnUNetTrainerV2_ReLU in 2-D; test_reference_import_variants.py checks every
fixture on the CPU).
Routes (2-D, spies on cineflow.ops): the ReLU, GeLU, LReLU(0.2), GN and BN networks hand norm + activation to the staging of the next
convolution at every layer where the stock network of the same shape does (here the four 3x3 pairs of the two upper levels), with the slope
the activation stands for (0, -1 = GELU, 0.2); the 1x1 head takes it where the stock one does, except under GELU, which
cf_norm_head_1x1 does not have.  A BN network asks no convolution for statistics and makes one table per layer; a Mish network and a
conv_nonlin_norm network defer nowhere.
End to end: the _BN 2-D folder through `python -m cineflow.predict` on a two-slice NIfTI; the label file equals the arg-max of the
sliding-window softmax stored in the fixture wherever its top two entries differ by more than the bar (a softmax within the tiled-softmax
bar 2e-5 of the stored one cannot flip those)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _variant_fixture as VF

pytestmark = pytest.mark.gpu

V = "nnUNetTrainerV2_"
_cache = {}


def imported(dim, name, tmp_path_factory):
    from cineflow import reference_models as R
    if (dim, name) not in _cache:
        base = tmp_path_factory.mktemp("%s_%s" % (dim, name[len(V):]))
        out = str(base / "model")
        R.import_reference_model_folder(VF.folder(dim, name, str(base / "ref")), None, out)
        _cache[(dim, name)] = out
    return _cache[(dim, name)]


def network(dim, name, dev, tmp_path_factory):
    from cineflow.predict import load_model_and_checkpoint_files
    trainer, params = load_model_and_checkpoint_files(imported(dim, name, tmp_path_factory), [0], device=dev)
    trainer.load_checkpoint_ram(params[0])
    return trainer.seg_net


@pytest.mark.parametrize("dim,name", VF.CASES)
def test_imported_variant_reproduces_the_reference_logits(dev, tmp_path_factory, dim, name):
    net = network(dim, name, dev, tmp_path_factory)
    x, ref = VF.expected(dim, name)
    logits = net(x.to(dev)).cpu()
    d = float((logits.double() - ref.double()).abs().max())
    tie = VF.near_tie(ref, VF.BAR)
    share = float(tie.double().mean())
    flips = int(((logits.argmax(1) != ref.argmax(1)) & ~tie).sum())
    print("\n  %s %-40s logits max|diff| %.3e   near ties %.4f %%   label flips outside them %d" % (dim, name, d, 100 * share, flips))
    assert share <= 0.01
    assert d <= VF.BAR, "%s %s: logits max|diff| %.3e" % (dim, name, d)
    assert flips == 0


# ------------------------------------------------------------------------------------------------------------------ routes
SPIED = ("conv2d_f16s_prenorm", "conv2d_wino_prenorm", "norm_head_1x1", "coef_apply", "group_norm", "group_norm_apply", "group_norm_coef",
         "batch_norm_coef", "conv2d_f16s", "conv2d_wino", "conv2d_small_cin", "conv_transpose2d_k2s2_f16s")


@pytest.fixture
def spy(monkeypatch):
    from cineflow import ops
    log = []

    def wrap(name, real):
        def f(*a, **k):
            log.append((name, a, k))
            return real(*a, **k)
        return f
    for name in SPIED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return log


def summary(log):
    n = {name: sum(1 for nm, _a, _k in log if nm == name) for name in SPIED}
    slopes = [a[2] for nm, a, _k in log if nm in ("conv2d_f16s_prenorm", "conv2d_wino_prenorm")]
    head_slopes = [a[2] for nm, a, _k in log if nm == "norm_head_1x1"]
    stats = [k.get("stats_groups") for nm, _a, k in log if nm in ("conv2d_f16s_prenorm", "conv2d_wino_prenorm", "conv2d_f16s", "conv2d_wino")]
    stats += [a[3] if len(a) > 3 else k.get("stats_groups") for nm, a, k in log if nm == "conv2d_small_cin"]
    return n, slopes, head_slopes, stats


@pytest.fixture(scope="module")
def stock_routes(dev):
    """(prenorm calls, head calls) of the stock Generic_UNet of the fixtures' shape on the fixtures' input: where the stock network defers"""
    from cineflow import ops
    from cineflow.models import Generic_UNet
    from cineflow.weights import seeded_state_dict
    net = Generic_UNet(1, 8, 4, 3, pool_op_kernel_sizes=[[2, 2], [2, 2], [2, 1]])
    net.load_state_dict(seeded_state_dict(net.state_shapes(), seed=3), dev)
    x = VF.expected("2d", V + "ReLU")[0].to(dev)
    count = {"pre": 0, "head": 0}
    real = {k: getattr(ops, k) for k in ("conv2d_f16s_prenorm", "conv2d_wino_prenorm", "norm_head_1x1")}
    try:
        for k, key in (("conv2d_f16s_prenorm", "pre"), ("conv2d_wino_prenorm", "pre"), ("norm_head_1x1", "head")):
            def f(*a, _k=k, _key=key, **kw):
                count[_key] += 1
                return real[_k](*a, **kw)
            setattr(ops, k, f)
        net(x)
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)
    assert count["pre"] >= 2 and count["head"] == 1, count          # 3x3 pairs of the two upper levels, and the head
    return count["pre"], count["head"]


@pytest.mark.parametrize("name,slope,head", [(V + "ReLU", 0.0, True), (V + "GeLU", -1.0, False), (V + "LReLU_slope_2en1", 0.2, True),
                                             (V + "GN", 0.01, True), (V + "BN", 0.01, True), (V + "ReLU_biasInSegOutput", 0.0, True),
                                             (V + "3ConvPerStageSameFilters", 0.01, True)])
def test_deferrable_variants_defer_where_the_stock_network_does(dev, tmp_path_factory, spy, stock_routes, name, slope, head):
    net = network("2d", name, dev, tmp_path_factory)
    x = VF.expected("2d", name)[0].to(dev)
    del spy[:]
    net(x)
    n, slopes, head_slopes, stats = summary(spy)
    pre = n["conv2d_f16s_prenorm"] + n["conv2d_wino_prenorm"]
    print("\n  %-40s prenorm %d (stock %d)  head %d (stock %d)  coef_apply %d  gn apply %d  gn %d" % (
        name, pre, stock_routes[0], n["norm_head_1x1"], stock_routes[1], n["coef_apply"], n["group_norm_apply"], n["group_norm"]))
    if name == V + "3ConvPerStageSameFilters":
        assert pre > stock_routes[0]                                 # a third convolution per stage: one more pair per deferring stack
    else:
        assert pre == stock_routes[0]
    assert slopes == [slope] * pre
    assert n["norm_head_1x1"] == (stock_routes[1] if head else 0) and head_slopes == [slope] * n["norm_head_1x1"]
    if name == V + "ReLU_biasInSegOutput":
        head_call = [(a, k) for nm, a, k in spy if nm == "norm_head_1x1"][0]
        assert (head_call[0][4] if len(head_call[0]) > 4 else head_call[1].get("bias")) is not None
    if name == V + "BN":
        assert not any(stats), stats                                 # no convolution is asked for statistics
        assert n["batch_norm_coef"] == 14 and n["group_norm"] == n["group_norm_apply"] == n["group_norm_coef"] == 0
        del spy[:]
        net(x)
        assert summary(spy)[0]["batch_norm_coef"] == 0               # the tables are kept per batch size
    else:
        assert n["batch_norm_coef"] == 0 and any(stats)


@pytest.mark.parametrize("name", [V + "Mish", V + "ReLU_convReLUIN", V + "lReLU_convReLUIN", V + "NoNormalization"])
def test_mish_other_order_and_no_norm_defer_nowhere(dev, tmp_path_factory, spy, name):
    net = network("2d", name, dev, tmp_path_factory)
    x = VF.expected("2d", name)[0].to(dev)
    del spy[:]
    net(x)
    n, _slopes, _hs, stats = summary(spy)
    print("\n  %-40s coef_apply %d  group_norm %d  group_norm_apply %d" % (name, n["coef_apply"], n["group_norm"], n["group_norm_apply"]))
    assert n["conv2d_f16s_prenorm"] == n["conv2d_wino_prenorm"] == n["norm_head_1x1"] == 0
    if "conv" in name[len(V):]:
        # conv, activation pass, then the norm on the activated map with its own statistics: no fused statistics, no activation in the norm
        assert n["coef_apply"] == 14 and n["group_norm"] == 14 and n["group_norm_apply"] == 0 and not any(stats)
        assert all(k.get("act") is None for nm, _a, k in spy if nm == "group_norm")
    else:
        assert n["coef_apply"] == 14 and n["group_norm"] == n["group_norm_apply"] == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_bn_folder_through_the_predict_command(dev, tmp_path_factory, tmp_path):
    from cineflow.nifti import read_nifti, write_nifti
    model = imported("2d", V + "BN", tmp_path_factory)
    e = torch.load(os.path.join(VF.TREE, "e2e_bn_2d.pt"), map_location="cpu", weights_only=True)
    inp, out = tmp_path / "in", tmp_path / "out"
    (inp / "patient001").mkdir(parents=True)
    write_nifti(str(inp / "patient001" / "patient001_frame00_0000.nii.gz"), e["volume"].numpy(), (1.5, 1.5, 8.0), (0, 0, 0))   # the stage's spacing
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "cardiac-segmentation-optical-flow_amd"), root, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "cineflow.predict", "-i", str(inp), "-o", str(out), "-m", model, "-f", "0",
                        "--num_threads_preprocessing", "1", "--num_threads_nifti_save", "1"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(out), "**", "patient001_frame00.nii.gz"), recursive=True)
    assert len(files) == 1, files
    labels = read_nifti(files[0])[0]
    ref = e["softmax"]                                                       # [K, Z, Y, X]
    tie = VF.near_tie(ref, VF.BAR, dim=0).numpy()
    want = ref.argmax(0).numpy()
    assert labels.shape == want.shape and float(tie.mean()) <= 0.01
    flips = int(((labels != want) & ~tie).sum())
    print("\n  _BN 2-D folder, predict command: %d voxels, near ties %.4f %%, label flips outside them %d" % (want.size, 100 * float(tie.mean()), flips))
    assert flips == 0
