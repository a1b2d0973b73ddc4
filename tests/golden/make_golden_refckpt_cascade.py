#!/usr/bin/env python3
"""Generate tests/golden/ref_model_folder_cascade/: the two model folders of an nnU-Net cascade (`3d_lowres` and `3d_cascade_fullres`) in
the layout the REFERENCE's trainers write, by running its own writers (make_golden_refckpt3d.py's route).

    cd /tmp && python <repo>/tests/golden/make_golden_refckpt_cascade.py

Needs the reference checkout (read-only; see _ref_import.py).  Only the data written here travels with the repository:

    ref_model_folder_cascade/plans.pkl                                   3-D planner layout with TWO stages: 0 = lowres (coarser spacing,
                                                                         patch (8, 32, 32)), 1 = fullres
    ref_model_folder_cascade/fold_0/model_final_checkpoint.model[.pkl]   Generic_UNet(1 + 3, ..., nn.Conv3d, ...), name nnUNetTrainerV2CascadeFullRes,
                                                                         init[5] = 1
    ref_model_folder_cascade/lowres/plans.pkl                            the same plans (the lowres trainer's folder holds its own copy)
    ref_model_folder_cascade/lowres/fold_0/model_final_checkpoint.*      Generic_UNet(1, ...), name nnUNetTrainer, init[5] = 0
    ref_model_folder_cascade/expected_outputs.pt                         tensors only: a seeded input [1,4,8,32,32] and the reference network's
                                                                         logits; a seeded label map, a target shape, seeded data on that grid
                                                                         and what the reference's preprocess_save (predict.py:61-85) returns

Both checkpoints are written by the reference's own `nnUNetTrainer.save_checkpoint` on objects that carry only the attributes it reads (the
cascade one on a subclass carrying the reference trainer's class name: nnUNetTrainerV2_CascadeFullRes.py:39).  `preprocess_save` runs in
place; SimpleITK is absent, so its two reads return the arrays generated here, and batchgenerators / skimage are absent, so
`resize_segmentation` / `resize` are the oracle's restatements (oracle/preprocess.py) injected into the reference module: parity unpinned
for these two.  The label map is smoothed noise quantised to 4 labels, chosen so that no resized indicator lies within 1e-4 of 0.5 (asserted
here): no voxel's label depends on rounding.  Every file's sha256 is compared with the tree already on disk.
"""
import collections
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "cardiac-segmentation-optical-flow_amd"))

import _ref_import  # noqa: E402

_ref_import.install()

from cineflow.weights import fill_module_  # noqa: E402
from make_golden_refckpt import digest, one_step, randn, write_pickle  # noqa: E402
from oracle import preprocess as OP  # noqa: E402

torch.set_num_threads(8)
TREE = os.path.join(HERE, "ref_model_folder_cascade")
TASK = "Task027_x"
PATCH = (8, 32, 32)
POOL = [[1, 2, 2], [2, 2, 2]]
KERN = [[1, 3, 3], [3, 3, 3], [3, 3, 3]]
BASE = 4
SEG_PREV_SHAPE, SEG_TARGET_SHAPE, SEG_PREV_SEED = (7, 19, 15), (10, 29, 23), 3
TIE_MARGIN = 1e-4
HEAD_SCALE = 4.0
REPORT = []


def reference_plans():
    """the plans dict ExperimentPlanner3D_v21.plan_experiment writes when it adds a low-resolution stage
    (experiment_planner_baseline_3DUNet.py:225-252, :343-357, :404-441): stage 0 is the coarser one, the last stage the full resolution"""
    def stage(spacing, median):
        return {"batch_size": np.int64(2), "num_pool_per_axis": [1, 2, 2], "patch_size": np.array(PATCH),
                "median_patient_size_in_voxels": np.array(median), "current_spacing": np.array(spacing),
                "original_spacing": np.array([10.0, 1.5, 1.5]), "do_dummy_2D_data_aug": True, "pool_op_kernel_sizes": POOL,
                "conv_kernel_sizes": KERN}
    ip = collections.OrderedDict([(0, collections.OrderedDict([("median", np.float64(98.5)), ("mean", np.float64(101.25)), ("sd", np.float64(40.0)),
                                                                ("mn", np.float64(0.0)), ("mx", np.float64(812.0)), ("percentile_99_5", np.float64(390.0)),
                                                                ("percentile_00_5", np.float64(2.0))]))])
    props = {"all_sizes": [(10, 40, 36), (9, 38, 36)], "all_spacings": [np.array([10.0, 1.5, 1.5]), np.array([10.0, 1.4, 1.4])],
             "all_classes": [1, 2, 3], "modalities": {0: "MRI"}, "intensityproperties": ip,
             "size_reductions": collections.OrderedDict([("patient001_frame01", np.float64(1.0)), ("patient002_frame01", np.float64(0.93))])}
    return {"num_stages": 2, "num_modalities": 1, "modalities": {0: "MRI"}, "normalization_schemes": collections.OrderedDict([(0, "nonCT")]),
            "dataset_properties": props, "list_of_npz_files": ["nnUNet_cropped_data/%s/patient001_frame01.npz" % TASK],
            "original_spacings": props["all_spacings"], "original_sizes": props["all_sizes"],
            "preprocessed_data_folder": "nnUNet_preprocessed/%s" % TASK, "num_classes": 3, "all_classes": [1, 2, 3], "base_num_features": BASE,
            "use_mask_for_norm": collections.OrderedDict([(0, False)]), "keep_only_largest_region": None, "min_region_size_per_class": None,
            "min_size_per_class": None, "transpose_forward": [np.int64(0), 1, 2],
            "transpose_backward": [np.int64(0), np.int64(1), np.int64(2)], "data_identifier": "nnUNetData_plans_v2.1",
            "plans_per_stage": {0: stage([10.0, 2.0, 2.0], [10, 30, 27]), 1: stage([10.0, 1.5, 1.5], [10, 40, 36])},
            "preprocessor_name": "GenericPreprocessor", "conv_per_stage": 2}


def save_with_stage(trainer_cls, network, optimizer, plans, stage, fname):
    """make_golden_refckpt.save_like_the_reference with the trainer's `stage` argument (init_args[5], nnUNetTrainer.py:60-62) set"""
    t = trainer_cls.__new__(trainer_cls)
    t.network, t.optimizer, t.lr_scheduler, t.amp_grad_scaler = network, optimizer, None, None
    t.epoch = 999
    t.all_tr_losses = [np.mean([0.9, 0.7]), np.mean([0.6, 0.5])]
    t.all_val_losses = [np.mean([0.8, 0.75]), np.mean([0.7, 0.55])]
    t.all_val_losses_tr_mode = []
    t.all_val_eval_metrics = [np.mean([0.61, 0.72, 0.8]), np.mean([0.7, 0.78, 0.86])]
    t.best_epoch_based_on_MA_tr_loss, t.best_MA_tr_loss_for_patience, t.best_val_eval_criterion_MA = 998, np.mean([0.55, 0.5]), np.mean([0.7, 0.8])
    t.init_args = ("nnUNet_preprocessed/%s/nnUNetPlansv2.1_plans_3D.pkl" % TASK, 0, "output", "nnUNet_preprocessed/" + TASK, True, stage, True, True,
                   False)
    t.plans = plans
    t.print_to_log_file = lambda *a, **k: None
    trainer_cls.save_checkpoint(t, fname)


def smoothed_labels(shape, seed, nlabels=4):
    """Gaussian-smoothed seeded noise quantised to `nlabels` labels of about equal volume (uint8)"""
    from scipy.ndimage import gaussian_filter
    g = gaussian_filter(np.random.RandomState(seed).randn(*shape), 1.5)
    edges = np.quantile(g, np.linspace(0, 1, nlabels + 1)[1:-1])
    return np.digitize(g, edges).astype(np.uint8)


def tie_margin(seg, new_shape):
    """min over the labels and voxels of |resized indicator - 0.5| (oracle, float64)"""
    return min(float(np.abs(OP.resize((seg == c).astype(float), new_shape, 1, mode="edge", clip=True, anti_aliasing=False) - 0.5).min())
               for c in np.unique(seg))


def reference_preprocess_save(data, seg_prev, classes):
    """the reference's preprocess_save (predict.py:61-85) in place: its preprocess_fn returns `data`, its two SimpleITK reads return `seg_prev`
    and an image of the same shape, `isfile` is true for the made-up label file name"""
    from nnunet.utilities.one_hot_encoding import to_one_hot
    # predict.py imports every trainer of the fork at module level; two of those imports cannot be satisfied here and neither is on the path
    # of preprocess_save: they get _ref_import's inert stand-ins
    _ref_import._STUB_ROOTS = tuple(_ref_import._STUB_ROOTS) + ("albumentations",)
    unused = "nnunet.training.network_training.nnMTLTrainerV2Flow_recursive_video"
    sys.modules.setdefault(unused, _ref_import._StubModule(unused))
    try:
        import nnunet.inference.predict as ref_predict
    except Exception as e:                                                   # (an import the image cannot satisfy)
        raise RuntimeError("cannot import the reference's nnunet.inference.predict in place (%s: %s)" % (type(e).__name__, e)) from e
    images = {"prev.nii.gz": seg_prev, "case_0000.nii.gz": np.zeros(seg_prev.shape, np.float32)}
    ref_predict.sitk = types.SimpleNamespace(ReadImage=lambda f: images[os.path.basename(f[0] if isinstance(f, (list, tuple)) else f)],
                                             GetArrayFromImage=lambda im: im)
    ref_predict.os = os                                                      # (names batchgenerators' star import supplies)
    ref_predict.isfile = lambda f: True
    ref_predict.resize_segmentation = OP.resize_segmentation
    ref_predict.to_one_hot = to_one_hot
    files = [[os.path.join("in", "patient", "case_0000.nii.gz")]]           # the fork hands preprocess_save a patient: one file list per frame
    _out, (d, _dct) = ref_predict.preprocess_save(lambda l_: (data, None, {}), files, [os.path.join("out", "case.nii.gz")],
                                                  os.path.join("lowres", "prev.nii.gz"), classes, [0, 1, 2])
    return d


def build(out):
    import nnunet.training.network_training.nnUNetTrainer as ref_trainer_mod
    from nnunet.network_architecture.generic_UNet import Generic_UNet
    from nnunet.network_architecture.initialization import InitWeights_He
    ref_trainer_mod.write_pickle = write_pickle
    nnUNetTrainer = ref_trainer_mod.nnUNetTrainer
    # the cascade trainer's save_checkpoint is nnUNetTrainer's (nnUNetTrainerV2_CascadeFullRes.py:39 -> nnUNetTrainerV2 -> nnUNetTrainer); what the
    # importer reads of it is the class NAME in the .model.pkl
    cascade_cls = type("nnUNetTrainerV2CascadeFullRes", (nnUNetTrainer,), {})
    plans = reference_plans()

    def unet(cin, seed):
        # nnUNetTrainerV2.py:147-169 with threeD = True
        net = Generic_UNet(cin, BASE, 4, len(POOL), 2, 2, torch.nn.Conv3d, torch.nn.InstanceNorm3d, {"eps": 1e-5, "affine": True}, torch.nn.Dropout3d,
                           {"p": 0, "inplace": True}, torch.nn.LeakyReLU, {"negative_slope": 1e-2, "inplace": True}, True, False, lambda x: x,
                           InitWeights_He(1e-2), POOL, KERN, False, True, True)
        fill_module_(net, seed)
        with torch.no_grad():                                                # seeded weights give an almost flat softmax, unlike a trained network:
            for n, p in net.named_parameters():                             # sharper heads keep the voxels whose arg-max hangs on the last bits
                if n.startswith("seg_outputs"):                             # of the softmax rare (tests/test_gpu_reference_import_cascade.py)
                    p.mul_(HEAD_SCALE)
        opt = torch.optim.SGD(net.parameters(), 0.01, weight_decay=3e-5, momentum=0.99, nesterov=True)
        one_step(opt, [p for n, p in net.named_parameters() if n.startswith("seg_outputs")])
        net.eval()
        net.do_ds = False
        return net, opt

    os.makedirs(os.path.join(out, "fold_0"))
    os.makedirs(os.path.join(out, "lowres", "fold_0"))
    write_pickle(plans, os.path.join(out, "plans.pkl"))
    write_pickle(plans, os.path.join(out, "lowres", "plans.pkl"))
    full, opt = unet(1 + 3, 92)                                              # nnUNetTrainerV2_CascadeFullRes.py:93: + (num_classes - 1) channels
    save_with_stage(cascade_cls, full, opt, plans, 1, os.path.join(out, "fold_0", "model_final_checkpoint.model"))
    low, opt = unet(1, 93)
    save_with_stage(nnUNetTrainer, low, opt, plans, 0, os.path.join(out, "lowres", "fold_0", "model_final_checkpoint.model"))

    with torch.no_grad():
        x = randn(1, 4, *PATCH, seed=95)
        x[:, 1:] = torch.nn.functional.one_hot(torch.from_numpy(smoothed_labels(PATCH, 96).astype(np.int64)), 4)[..., 1:].permute(3, 0, 1, 2).float()
        logits = full(x)
    REPORT.append("reference cascade Generic_UNet(1 + 3, conv_op=nn.Conv3d) logits %s, mean |logit| %.4f" % (tuple(logits.shape), float(logits.abs().mean())))

    seg_prev = smoothed_labels(SEG_PREV_SHAPE, SEG_PREV_SEED)
    margin = tie_margin(seg_prev, SEG_TARGET_SHAPE)
    assert margin >= TIE_MARGIN, margin
    data = randn(1, *SEG_TARGET_SHAPE, seed=98).numpy()
    d = reference_preprocess_save(data, seg_prev, [1, 2, 3])
    assert d.shape == (4,) + SEG_TARGET_SHAPE and d.dtype == np.float32
    unl = float((d[1:].sum(0) == 0).mean()) - float((OP.resize_segmentation(seg_prev, SEG_TARGET_SHAPE, 1) == 0).mean())
    assert unl == 0.0
    REPORT.append("preprocess_save %s -> %s: min |indicator - 0.5| = %.3e (>= %.0e asserted), one-hot planes cover %.4f of the grid"
                  % (SEG_PREV_SHAPE, SEG_TARGET_SHAPE, margin, TIE_MARGIN, float(d[1:].sum(0).mean())))
    REPORT.append("resize_segmentation / resize inside preprocess_save: the oracle's restatements (batchgenerators, skimage absent): parity unpinned for these two")
    torch.save({"seg_x": x.contiguous(), "seg_logits": logits.contiguous(), "prev_seg": torch.from_numpy(seg_prev),
                "prev_target_shape": torch.tensor(SEG_TARGET_SHAPE), "prev_data": torch.from_numpy(data),
                "prev_input": torch.from_numpy(np.ascontiguousarray(d))}, os.path.join(out, "expected_outputs.pt"))


def main():
    before = digest(TREE) if os.path.isdir(TREE) else None
    tmp = tempfile.mkdtemp()
    try:
        new = os.path.join(tmp, "ref_model_folder_cascade")
        build(new)
        after = digest(new)
        for rel, (_h, n) in after.items():
            assert n <= 1000000, (rel, n)
        if os.path.isdir(TREE):
            shutil.rmtree(TREE)
        shutil.copytree(new, TREE)
    finally:
        shutil.rmtree(tmp)
    if before is None:
        verdict = "first generation (no tree on disk to compare with)"
    elif before == after:
        verdict = "reproduced the tree on disk bit for bit (%d files, sha256 identical)" % len(after)
    else:
        verdict = "DIFFERS from the tree on disk: %s" % sorted(k for k in set(before) | set(after) if before.get(k) != after.get(k))
    print(verdict)
    with open(os.path.join(HERE, "PIN_REPORT_refckpt_cascade.txt"), "w") as f:
        f.write("tests/golden/ref_model_folder_cascade (generated by make_golden_refckpt_cascade.py from the reference's own save_checkpoint / write_pickle /\n"
                "preprocess_save)\n")
        f.write("checkpoint route: nnUNetTrainer.save_checkpoint -> NetworkTrainer.save_checkpoint on objects carrying only the attributes they read;\n"
                "cascade stage: class name nnUNetTrainerV2CascadeFullRes, init[5] = 1; lowres stage: nnUNetTrainer, init[5] = 0\n")
        for line in REPORT:
            f.write(line + "\n")
        for rel in sorted(after):
            f.write("%-62s %8d bytes  sha256 %s\n" % (rel, after[rel][1], after[rel][0]))
        f.write("total %d bytes\n" % sum(n for _h, n in after.values()))
        f.write("rerun: %s\n" % verdict)


if __name__ == "__main__":
    main()
