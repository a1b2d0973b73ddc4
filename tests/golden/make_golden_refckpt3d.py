#!/usr/bin/env python3
"""Generate tests/golden/ref_model_folder_3d/: a `3d_fullres` model folder in the layout the REFERENCE's trainer writes, by running its
own writers (make_golden_refckpt.py's route, for the 3-D network).

    cd /tmp && python <repo>/tests/golden/make_golden_refckpt3d.py

Needs the reference checkout (read-only; see _ref_import.py).  Only the data written here travels with the repository:

    ref_model_folder_3d/plans.pkl                                   3-D experiment-planner layout (numpy arrays and scalars, 3-entry patch_size)
    ref_model_folder_3d/fold_0/model_final_checkpoint.model[.pkl]   reduced-width Generic_UNet(conv_op = nn.Conv3d), saved through nn.DataParallel
    ref_model_folder_3d/expected_outputs.pt                         a seeded input [1,1,8,32,32] and the reference's logits (tensors only)

The checkpoint is written by the reference's own `nnUNetTrainer.save_checkpoint` (-> `NetworkTrainer.save_checkpoint`, torch.save, then
`write_pickle` of {init, name, class, plans}) on an nnUNetTrainer object that carries only the attributes those two methods read; the
optimizer (SGD, nnUNetTrainerV2's settings) took one real step.  Base width 4 and two pooling stages ((1,2,2) then (2,2,2); (1,3,3)
kernels in the first stage, (3,3,3) after) keep every file far below the size limit of a committed file.  Every file's sha256 is
compared with the tree already on disk: PIN_REPORT_refckpt3d.txt says whether this run reproduced it bit for bit.
"""
import collections
import hashlib
import os
import pickle
import shutil
import sys
import tempfile

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
from make_golden_refckpt import digest, one_step, randn, save_like_the_reference, write_pickle  # noqa: E402

torch.set_num_threads(8)
TREE = os.path.join(HERE, "ref_model_folder_3d")
TASK = "Task027_x"
PATCH = (8, 32, 32)
POOL = [[1, 2, 2], [2, 2, 2]]
KERN = [[1, 3, 3], [3, 3, 3], [3, 3, 3]]
BASE = 4
REPORT = []


def reference_plans():
    """the plans dict ExperimentPlanner3D_v21.plan_experiment writes (experiment_planner_baseline_3DUNet.py:225-252, :343-357), one stage
    (the data set is small enough that the planner adds no low-resolution stage), with the numpy types its arithmetic produces"""
    stage = {"batch_size": np.int64(2), "num_pool_per_axis": [1, 2, 2], "patch_size": np.array(PATCH),
             "median_patient_size_in_voxels": np.array([10, 40, 36]), "current_spacing": np.array([10.0, 1.5, 1.5]),
             "original_spacing": np.array([10.0, 1.5, 1.5]), "do_dummy_2D_data_aug": True, "pool_op_kernel_sizes": POOL,
             "conv_kernel_sizes": KERN}
    ip = collections.OrderedDict([(0, collections.OrderedDict([("median", np.float64(98.5)), ("mean", np.float64(101.25)), ("sd", np.float64(40.0)),
                                                                ("mn", np.float64(0.0)), ("mx", np.float64(812.0)), ("percentile_99_5", np.float64(390.0)),
                                                                ("percentile_00_5", np.float64(2.0))]))])
    props = {"all_sizes": [(10, 40, 36), (9, 38, 36)], "all_spacings": [np.array([10.0, 1.5, 1.5]), np.array([10.0, 1.4, 1.4])],
             "all_classes": [1, 2, 3], "modalities": {0: "MRI"}, "intensityproperties": ip,
             "size_reductions": collections.OrderedDict([("patient001_frame01", np.float64(1.0)), ("patient002_frame01", np.float64(0.93))])}
    return {"num_stages": 1, "num_modalities": 1, "modalities": {0: "MRI"}, "normalization_schemes": collections.OrderedDict([(0, "nonCT")]),
            "dataset_properties": props, "list_of_npz_files": ["nnUNet_cropped_data/%s/patient001_frame01.npz" % TASK],
            "original_spacings": props["all_spacings"], "original_sizes": props["all_sizes"],
            "preprocessed_data_folder": "nnUNet_preprocessed/%s" % TASK, "num_classes": 3, "all_classes": [1, 2, 3], "base_num_features": BASE,
            "use_mask_for_norm": collections.OrderedDict([(0, False)]), "keep_only_largest_region": None, "min_region_size_per_class": None,
            "min_size_per_class": None, "transpose_forward": [np.int64(0), 1, 2],
            "transpose_backward": [np.int64(0), np.int64(1), np.int64(2)], "data_identifier": "nnUNetData_plans_v2.1",
            "plans_per_stage": {0: stage}, "preprocessor_name": "GenericPreprocessor", "conv_per_stage": 2}


def build(out):
    import nnunet.training.network_training.nnUNetTrainer as ref_trainer_mod
    from nnunet.network_architecture.generic_UNet import Generic_UNet
    from nnunet.network_architecture.initialization import InitWeights_He
    ref_trainer_mod.write_pickle = write_pickle
    nnUNetTrainer = ref_trainer_mod.nnUNetTrainer
    plans = reference_plans()
    os.makedirs(os.path.join(out, "fold_0"))
    write_pickle(plans, os.path.join(out, "plans.pkl"))
    # nnUNetTrainerV2.py:147-169 with threeD = True
    unet = Generic_UNet(1, BASE, 4, len(POOL), 2, 2, torch.nn.Conv3d, torch.nn.InstanceNorm3d, {"eps": 1e-5, "affine": True}, torch.nn.Dropout3d,
                        {"p": 0, "inplace": True}, torch.nn.LeakyReLU, {"negative_slope": 1e-2, "inplace": True}, True, False, lambda x: x,
                        InitWeights_He(1e-2), POOL, KERN, False, True, True)
    fill_module_(unet, 81)
    opt = torch.optim.SGD(unet.parameters(), 0.01, weight_decay=3e-5, momentum=0.99, nesterov=True)
    one_step(opt, [p for n, p in unet.named_parameters() if n.startswith("seg_outputs")])
    unet.eval()
    unet.do_ds = False
    save_like_the_reference(nnUNetTrainer, torch.nn.DataParallel(unet), opt, plans, "nnUNet_preprocessed/" + TASK,
                            os.path.join(out, "fold_0", "model_final_checkpoint.model"))
    with torch.no_grad():
        x = randn(1, 1, *PATCH, seed=83)
        logits = unet(x)
    REPORT.append("reference Generic_UNet(conv_op=nn.Conv3d) logits %s, mean |logit| %.4f" % (tuple(logits.shape), float(logits.abs().mean())))
    torch.save({"seg_x": x.contiguous(), "seg_logits": logits.contiguous()}, os.path.join(out, "expected_outputs.pt"))


def main():
    before = digest(TREE) if os.path.isdir(TREE) else None
    tmp = tempfile.mkdtemp()
    try:
        new = os.path.join(tmp, "ref_model_folder_3d")
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
    with open(os.path.join(HERE, "PIN_REPORT_refckpt3d.txt"), "w") as f:
        f.write("tests/golden/ref_model_folder_3d (generated by make_golden_refckpt3d.py from the reference's own save_checkpoint / write_pickle)\n")
        f.write("checkpoint route: nnUNetTrainer.save_checkpoint -> NetworkTrainer.save_checkpoint on an nnUNetTrainer object carrying only the\n"
                "attributes they read; state_dict saved through nn.DataParallel\n")
        for line in REPORT:
            f.write(line + "\n")
        for rel in sorted(after):
            f.write("%-62s %8d bytes  sha256 %s\n" % (rel, after[rel][1], after[rel][0]))
        f.write("total %d bytes\n" % sum(n for _h, n in after.values()))
        f.write("rerun: %s\n" % verdict)


if __name__ == "__main__":
    main()
