#!/usr/bin/env python3
"""Generate tests/golden/ref_model_folder_mtl/: a model folder in the layout the REFERENCE's nnMTLTrainerV2 writes, by its own writers.

    cd /tmp && python <repo>/tests/golden/make_golden_mtl_folder.py

Needs the reference checkout (read-only; see _ref_import.py).  Only the data written here travels with the repository:

    ref_model_folder_mtl/seg/plans.pkl                                   2-D experiment-planner layout (make_golden_refckpt.reference_plans)
    ref_model_folder_mtl/seg/fold_{0,1}/model_final_checkpoint.model[.pkl]   reduced-width 4-class MTLmodel on the 64 x 64 crop
    ref_model_folder_mtl/seg_config.yaml                                 seg_model.yaml's values: reduced widths, patch_size [96, 96], cropper true
    ref_model_folder_mtl/binary/model_final_checkpoint.model[.pkl]       the 2-class MTLmodel cropper on the 96 x 96 image (nnMTLTrainerV2.py:601)
    ref_model_folder_mtl/cropping_config.yaml                            adversarial_acdc.yaml's values at the same reduced widths

A checkpoint is larger than a committed file may be, so each is stored as `<name>.gz.part<i>` (see `pack`); tests/_mtl_folder_fixture.py
restores the reference's bytes.

The networks are the reference's own `MTLmodel` (make_golden_mtl.build_reference) at the widths tests/test_mtl.py calls RED, image 96,
crop 64, window 8.  The checkpoints are written by the reference's own `nnUNetTrainer.save_checkpoint` (-> `NetworkTrainer.save_checkpoint`,
torch.save, then write_pickle of {init, name, class, plans}), which nnMTLTrainerV2 inherits unchanged.  The module nnMTLTrainerV2.py itself
does not import in the reference snapshot (nnunet/lib/training_utils.py imports names its lib/utils.py lacks), so the object that method
runs on is an instance of an EMPTY subclass of the reference's nnUNetTrainer that carries the trainer's name -- the one thing of the
class that reaches the file ('name' / 'class' in .model.pkl) -- and only the attributes the two methods read.

The oracle (oracle/mtl.py) is pinned against every reference network on seeded inputs, and every file's sha256 is compared with the tree
already on disk: PIN_REPORT_refckpt_mtl.txt says whether this run reproduced it bit for bit.
"""
import copy
import gzip
import os
import shutil
import sys
import tempfile

import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_refckpt as R  # noqa: E402  (installs the reference import, puts the repository on sys.path)
import make_golden_mtl as GM  # noqa: E402

from cineflow.weights import fill_module_  # noqa: E402
from oracle import mtl as OMTL  # noqa: E402

TREE = os.path.join(HERE, "ref_model_folder_mtl")
IMAGE, CROP, WINDOW = 96, 64, 8
RED = dict(in_dims=[1, 16, 32], out_encoder_dims=[8, 16, 32], conv_depth=[2, 2, 2], spatial_cross_attention_num_heads=[2, 2, 4], bottleneck_heads=8)
REDUCED_YAML = dict(in_encoder_dims=RED["in_dims"], out_encoder_dims=RED["out_encoder_dims"], conv_depth=RED["conv_depth"],
                    spatial_cross_attention_num_heads=RED["spatial_cross_attention_num_heads"], bottleneck_heads=RED["bottleneck_heads"],
                    patch_size=[IMAGE, IMAGE])
SEEDS = {"fold_0": 81, "fold_1": 82, "binary": 83}


def reduced_config(name, **more):
    with open(os.path.join(R._ref_import.REFERENCE_ROOT, "nnunet", name)) as f:
        cfg = yaml.safe_load(f)
    cfg.update(copy.deepcopy(REDUCED_YAML))
    cfg.update(more)
    return cfg


def reference_net(image, ncls, seed):
    net = fill_module_(GM.build_reference(image, WINDOW, ncls, RED["in_dims"], RED["out_encoder_dims"], RED["spatial_cross_attention_num_heads"],
                                          RED["bottleneck_heads"]), seed)
    return net


def save(trainer_cls, net, plans, fname):
    opt = torch.optim.SGD(net.parameters(), 0.01, weight_decay=3e-5, momentum=0.99, nesterov=True)
    R.one_step(opt, [p for n, p in net.named_parameters() if n.startswith("decoder.layers.2.")][:2])
    net.eval()
    net.do_ds = False
    os.makedirs(os.path.dirname(fname), exist_ok=True)
    R.save_like_the_reference(trainer_cls, net, opt, plans, "nnUNet_preprocessed/" + R.TASK, fname)


def pin_against_oracle(name, net, image, ncls, seed):
    ora = OMTL.MTLmodel(image, WINDOW, ncls, **RED).eval()
    ora.load_state_dict(net.state_dict(), strict=True)
    x = R.randn(2, 1, image, image, seed=seed)
    with torch.no_grad():
        R.pin(name, net(x)["pred"], ora(x)["pred"], 1e-5)


def build(out):
    import nnunet.training.network_training.nnUNetTrainer as ref_trainer_mod
    ref_trainer_mod.write_pickle = R.write_pickle
    nnMTLTrainerV2 = type("nnMTLTrainerV2", (ref_trainer_mod.nnUNetTrainer,), {})      # the name alone: see the module docstring
    plans = R.reference_plans()
    seg_dir = os.path.join(out, "seg")
    os.makedirs(seg_dir)
    R.write_pickle(plans, os.path.join(seg_dir, "plans.pkl"))
    with open(os.path.join(out, "seg_config.yaml"), "w") as f:
        yaml.safe_dump(reduced_config("seg_model.yaml", cropper=True), f, sort_keys=False)
    with open(os.path.join(out, "cropping_config.yaml"), "w") as f:
        yaml.safe_dump(reduced_config("adversarial_acdc.yaml"), f, sort_keys=False)
    for fold in (0, 1):
        net = reference_net(CROP, 4, SEEDS["fold_%d" % fold])
        save(nnMTLTrainerV2, net, plans, os.path.join(seg_dir, "fold_%d" % fold, "model_final_checkpoint.model"))
        pin_against_oracle("MTLmodel 4 classes, fold %d (imported fixture)" % fold, net, CROP, 4, 90 + fold)
    net = reference_net(IMAGE, 2, SEEDS["binary"])
    save(nnMTLTrainerV2, net, plans, os.path.join(out, "binary", "model_final_checkpoint.model"))
    pin_against_oracle("MTLmodel 2 classes, the cropper (imported fixture)", net, IMAGE, 2, 92)


PART = 900000


def pack(tree):
    """A file above the size limit of a committed file (the checkpoints: 1.3 MB of weights plus the Swin shift masks the reference's
    state_dict holds as buffers) is stored as <name>.gz.part0, .part1, ...: the gzip stream (level 9, no time stamp) of the bytes the
    reference wrote, cut into pieces.  tests/_mtl_folder_fixture.py joins and inflates them; the sha256 of the original bytes is in the
    pin report.  Returns {relative name: (sha256, size)} of the ORIGINAL files."""
    original = R.digest(tree)
    for rel, (_h, n) in original.items():
        if n > PART:
            path = os.path.join(tree, rel)
            with open(path, "rb") as f:
                z = gzip.compress(f.read(), 9, mtime=0)
            os.remove(path)
            for i in range(0, len(z), PART):
                with open("%s.gz.part%d" % (path, i // PART), "wb") as f:
                    f.write(z[i:i + PART])
    return original


def main():
    before = R.digest(TREE) if os.path.isdir(TREE) else None
    tmp = tempfile.mkdtemp()
    try:
        new = os.path.join(tmp, "ref_model_folder_mtl")
        build(new)
        original = pack(new)
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
    with open(os.path.join(HERE, "PIN_REPORT_refckpt_mtl.txt"), "w") as f:
        f.write("tests/golden/ref_model_folder_mtl (generated by make_golden_mtl_folder.py from the reference's own MTLmodel, save_checkpoint and write_pickle)\n")
        f.write("checkpoint route: nnUNetTrainer.save_checkpoint -> NetworkTrainer.save_checkpoint (nnMTLTrainerV2 inherits both) on an instance of an\n"
                "empty subclass named nnMTLTrainerV2 carrying only the attributes they read; nnMTLTrainerV2.py itself does not import in the snapshot\n")
        for line in R.REPORT:
            f.write(line + "\n")
        for rel in sorted(after):
            f.write("%-62s %8d bytes  sha256 %s\n" % (rel, after[rel][1], after[rel][0]))
        f.write("total %d bytes\n" % sum(n for _h, n in after.values()))
        for rel in sorted(original):
            if original[rel][1] > PART:
                f.write("before gzip + split: %-42s %8d bytes  sha256 %s\n" % (rel, original[rel][1], original[rel][0]))
        f.write("rerun: %s\n" % verdict)


if __name__ == "__main__":
    main()
