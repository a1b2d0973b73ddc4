#!/usr/bin/env python3
"""Generate tests/golden/ref_model_variants/: model folders of the REFERENCE's architectural trainer variants
(nnunet/training/network_training/nnUNet_variants/architectural_variants/), written by its own writers, with its own outputs.

    cd /tmp && python <repo>/tests/golden/make_golden_variants.py

Needs the reference checkout (read-only; see _ref_import.py).  Only the data written here travels with the repository.

For every trainer of TRAINERS, in 2-D and in 3-D, the network is built by that trainer's OWN `initialize_network`, called on an object of
the trainer's class that carries only the attributes the method reads (threeD, num_input_channels, base_num_features, num_classes,
net_num_pool_op_kernel_sizes, net_conv_kernel_sizes, conv_per_stage).  The weights are the seeded fill of cineflow.weights (BatchNorm
running statistics included: means around 0, variances away from 1), the optimizer (SGD, nnUNetTrainerV2's settings) takes one real step,
the network is left in eval mode, and the checkpoint is written by `nnUNetTrainer.save_checkpoint` (-> NetworkTrainer.save_checkpoint,
torch.save, then write_pickle of {init, name, class, plans}) on that same object: `.model.pkl` holds the trainer's real class name.

    2-D  base 8, pooling (2,2), (2,2), (2,1), input [2, 1, 48, 40]
    3-D  base 4, pooling (1,2,2), (2,2,2), kernels (1,3,3), (3,3,3), (3,3,3), input [1, 1, 6, 24, 20]

Layout (tests/_variant_fixture.py puts a trainer's folder back together):

    plans_2d.pkl, plans_3d.pkl                          the planners' layouts (make_golden_refckpt / make_golden_refckpt3d), patch = the input
    plans_3d_base8.pkl                                  ... for the 3-D GroupNorm network: 8 groups need 8 channels, so it alone has base 8
    inputs.pt                                           {'2d': x, '3d': x}: one seeded input per dimension
    models/<sha256[:16]>.model                          the checkpoints.  Trainers whose networks hold the same tensors (the activation and
                                                        the order of operations are not in a state_dict) write byte-identical files, kept once
    <2d|3d>/<trainer>/model_final_checkpoint.model.pkl  that trainer's pickle
    <2d|3d>/<trainer>/logits.pt                         the reference network's fp32 logits on the input
    e2e_bn_2d.pt                                        nnUNetTrainerV2_BN, 2-D: a seeded two-slice volume, preprocessed as the plans ask (oracle/preprocess.py),
                                                        and the sliding-window softmax (Gaussian, mirroring) of the reference's network on it
    index.json                                          trainer -> checkpoint file, and per trainer the share of voxels whose top-two logits lie
                                                        within the logits bar (1e-4) of each other

PIN_REPORT_variants.txt lists every file's sha256 and says whether this run reproduced the tree on disk.
"""
import copy
import importlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_refckpt as R  # noqa: E402  (installs the reference import, puts the repository on sys.path)
import make_golden_refckpt3d as R3  # noqa: E402

from cineflow.weights import fill_module_  # noqa: E402

torch.set_num_threads(8)
TREE = os.path.join(HERE, "ref_model_variants")
VARIANTS = "nnunet.training.network_training.nnUNet_variants.architectural_variants."
# class name -> module (file) name where they differ
MODULE_OF = {"nnUNetTrainerV2_lReLU_convReLUIN": "nnUNetTrainerV2_lReLU_convlReLUIN",
             "nnUNetTrainerV2_3ConvPerStageSameFilters": "nnUNetTrainerV2_3ConvPerStage_samefilters"}
TRAINERS = ("nnUNetTrainerV2_ReLU", "nnUNetTrainerV2_GeLU", "nnUNetTrainerV2_Mish", "nnUNetTrainerV2_LReLU_slope_2en1", "nnUNetTrainerV2_GN",
            "nnUNetTrainerV2_BN", "nnUNetTrainerV2_NoNormalization", "nnUNetTrainerV2_ReLU_convReLUIN", "nnUNetTrainerV2_lReLU_convReLUIN",
            "nnUNetTrainerV2_ReLU_biasInSegOutput", "nnUNetTrainerV2_3ConvPerStageSameFilters")
DIMS = {
    "2d": dict(threeD=False, base=8, pool=[[2, 2], [2, 2], [2, 1]], kern=[[3, 3]] * 4, shape=(2, 1, 48, 40), task=R.TASK),
    "3d": dict(threeD=True, base=4, pool=[[1, 2, 2], [2, 2, 2]], kern=[[1, 3, 3], [3, 3, 3], [3, 3, 3]], shape=(1, 1, 6, 24, 20), task=R3.TASK),
}
# MyGroupNorm(num_groups=8) cannot be built on 4 channels: the 3-D GroupNorm network alone has base 8 (and plans of its own)
BASE_OF = {("3d", "nnUNetTrainerV2_GN"): 8}
WEIGHT_SEED = {"2d": 171, "3d": 181}
INPUT_SEED = {"2d": 173, "3d": 183}
BAR = 1e-4            # the logits bar of tests/test_gpu_models.py for the reduced-width Generic_UNet fixtures
REPORT = []


def plans_for(dim, base=None):
    d = DIMS[dim]
    if dim == "2d":
        p = R.reference_plans()
        st = p["plans_per_stage"][0]
        st["patch_size"] = np.array(d["shape"][2:])
        st["num_pool_per_axis"] = [3, 2]
    else:
        p = R3.reference_plans()
        st = p["plans_per_stage"][0]
        st["patch_size"] = np.array(d["shape"][2:])
    st["pool_op_kernel_sizes"], st["conv_kernel_sizes"] = copy.deepcopy(d["pool"]), copy.deepcopy(d["kern"])
    p["base_num_features"] = base or d["base"]
    return p


def trainer_class(name):
    return getattr(importlib.import_module(VARIANTS + MODULE_OF.get(name, name)), name)


def build_network(cls, dim):
    """the trainer's own initialize_network on an object with the attributes it reads"""
    d = DIMS[dim]
    t = cls.__new__(cls)
    t.threeD, t.num_input_channels, t.base_num_features, t.num_classes = d["threeD"], 1, BASE_OF.get((dim, cls.__name__), d["base"]), 4
    t.net_num_pool_op_kernel_sizes, t.net_conv_kernel_sizes, t.conv_per_stage = copy.deepcopy(d["pool"]), copy.deepcopy(d["kern"]), 2
    cls.initialize_network(t)
    return t.network


def lift_last_block(net):
    """At base 4 the last block has four channels, and under ReLU all four are <= 0 on about 6 % of the voxels whatever the seed: the
    bias-free heads then give four logits of exactly 0, a tie.  The last block's shift (its norm's beta; without a norm its convolution's
    bias) is raised by 1 so that the share of such voxels falls under the 1 % the tests allow.  A tensor of the checkpoint like any other."""
    blk = net.conv_blocks_localization[-1][-1].blocks[-1]
    target = blk.instnorm.bias if getattr(blk.instnorm, "bias", None) is not None else blk.conv.bias
    with torch.no_grad():
        target += 1.0


def near_tie_share(logits, bar=BAR):
    top = torch.topk(logits.double(), 2, dim=1).values
    return float(((top[:, 0] - top[:, 1]) <= bar).double().mean())


def e2e_bn_2d(net, plans):
    """a two-slice volume through the plans' preprocessing (non-CT z-score over the volume, no resampling: the file's spacing is the
    stage's) and the sliding window of _internal_predict_3D_2Dconv_tiled around the REFERENCE's network: half-patch steps, Gaussian
    weighting, mirroring over both axes, on the CPU.  The window loop is oracle.models.predict_3d_2dconv_tiled (pinned against the
    reference's pieces by make_golden.py): the snapshot's own 2-D loop passes its mirror routine a `normalize` argument that routine
    does not take (neural_network.py:718 / :573) and cannot run."""
    g = torch.Generator().manual_seed(191)
    vol = (torch.randn(2, 60, 52, generator=g) * 40 + 100).numpy().astype(np.float32)             # [Z, Y, X] as the NIfTI is written
    data = ((vol - vol.mean()) / (vol.std() + 1e-8)).astype(np.float32)[None]                      # preprocessing.py:226-232 (nonCT)
    patch = tuple(int(v) for v in plans["plans_per_stage"][0]["patch_size"])
    net.do_ds = False
    from oracle import models as OM
    with torch.no_grad():
        seg, softmax = OM.predict_3d_2dconv_tiled(net, data, patch, step_size=0.5, do_mirroring=True, mirror_axes=(0, 1), use_gaussian=True,
                                                  pad_border_mode="constant", pad_kwargs={"constant_values": 0})
    sm = torch.from_numpy(np.ascontiguousarray(softmax)).float()
    top = torch.topk(sm.double(), 2, dim=0).values
    REPORT.append("e2e nnUNetTrainerV2_BN 2-D: volume %s, softmax top-two gap <= 1e-3 on %.4f %% of the voxels"
                  % (vol.shape, 100 * float(((top[0] - top[1]) <= 1e-3).double().mean())))
    return {"volume": torch.from_numpy(vol), "preprocessed": torch.from_numpy(data), "softmax": sm, "seg": torch.from_numpy(seg.astype(np.uint8))}


def build(out):
    import nnunet.training.network_training.nnUNetTrainer as ref_trainer_mod
    ref_trainer_mod.write_pickle = R.write_pickle
    os.makedirs(os.path.join(out, "models"))
    index, inputs = {}, {}
    for dim in ("2d", "3d"):
        stock_plans = plans_for(dim)
        R.write_pickle(stock_plans, os.path.join(out, "plans_%s.pkl" % dim))
        x = R.randn(*DIMS[dim]["shape"], seed=INPUT_SEED[dim]).contiguous()
        inputs[dim] = x
        index[dim] = {}
        for name in TRAINERS:
            cls = trainer_class(name)
            plans, plans_file = stock_plans, "plans_%s.pkl" % dim
            if (dim, name) in BASE_OF:
                plans, plans_file = plans_for(dim, BASE_OF[(dim, name)]), "plans_%s_base%d.pkl" % (dim, BASE_OF[(dim, name)])
                R.write_pickle(plans, os.path.join(out, plans_file))
            net = fill_module_(build_network(cls, dim), WEIGHT_SEED[dim])
            if dim == "3d":
                lift_last_block(net)
            opt = torch.optim.SGD(net.parameters(), 0.01, weight_decay=3e-5, momentum=0.99, nesterov=True)
            R.one_step(opt, [p for n, p in net.named_parameters() if n.startswith("seg_outputs")])
            net.eval()
            net.do_ds = False
            folder = os.path.join(out, dim, name)
            os.makedirs(folder)
            fname = os.path.join(folder, "model_final_checkpoint.model")
            R.save_like_the_reference(cls, torch.nn.DataParallel(net), opt, plans, "nnUNet_preprocessed/" + DIMS[dim]["task"], fname)
            sha = R.hashlib.sha256(open(fname, "rb").read()).hexdigest()[:16]
            kept = os.path.join(out, "models", sha + ".model")
            if os.path.exists(kept):
                os.remove(fname)
            else:
                shutil.move(fname, kept)
            with torch.no_grad():
                logits = net(x).contiguous()
            assert logits.shape == (x.shape[0], 4) + tuple(x.shape[2:]) and bool(torch.isfinite(logits).all())
            torch.save({"logits": logits}, os.path.join(folder, "logits.pt"))
            share = near_tie_share(logits)
            assert share <= 0.01, (dim, name, share)
            index[dim][name] = {"model": sha + ".model", "plans": plans_file, "near_tie_share": share}
            REPORT.append("%s %-44s checkpoint %s  mean |logit| %.4f  top-two gap <= %.0e on %.4f %% of the voxels"
                          % (dim, name, sha, float(logits.abs().mean()), BAR, 100 * share))
            print("  " + REPORT[-1])
            if dim == "2d" and name == "nnUNetTrainerV2_BN":
                torch.save(e2e_bn_2d(net, stock_plans), os.path.join(out, "e2e_bn_2d.pt"))
    torch.save(inputs, os.path.join(out, "inputs.pt"))
    with open(os.path.join(out, "index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)


def main():
    before = R.digest(TREE) if os.path.isdir(TREE) else None
    tmp = tempfile.mkdtemp()
    try:
        new = os.path.join(tmp, "ref_model_variants")
        build(new)
        after = R.digest(new)
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
    with open(os.path.join(HERE, "PIN_REPORT_variants.txt"), "w") as f:
        f.write("tests/golden/ref_model_variants (generated by make_golden_variants.py: each trainer's own initialize_network, the reference's own\n"
                "save_checkpoint / write_pickle)\n")
        for line in REPORT:
            f.write(line + "\n")
        for rel in sorted(after):
            f.write("%-70s %8d bytes  sha256 %s\n" % (rel, after[rel][1], after[rel][0]))
        f.write("total %d bytes\n" % sum(n for _h, n in after.values()))
        f.write("rerun: %s\n" % verdict)


if __name__ == "__main__":
    main()
