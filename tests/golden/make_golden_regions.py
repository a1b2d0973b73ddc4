#!/usr/bin/env python3
"""Generate tests/golden/ref_model_regions/: model folders of the REFERENCE's region-based trainer nnUNetTrainerV2BraTSRegions
(competitions_with_custom_Trainers/BraTS2020), written by its own writers, with its own sliding-window outputs.

    cd /tmp && python <repo>/tests/golden/make_golden_regions.py

Needs the reference checkout (read-only; see _ref_import.py).  Only the data written here travels with the repository.

In 2-D and in 3-D the network is built by the trainer's OWN `initialize_network` (which sets inference_apply_nonlin = nn.Sigmoid()), called
on an object of the trainer's class that carries only the attributes the method reads; 2 modalities, 3 region channels
(num_classes = len(get_brats_regions())).  Weights: the seeded fill of cineflow.weights, one real SGD step, eval mode; the rows of the
bias-free full-resolution head are then redrawn, row by row with rising seeds, until every region's sliding-window probability is above 0.5 on 10-90 % of the
fixture's voxels (a plain draw leaves a channel almost always or almost never above the threshold, and a label test on it would see one
label).  The checkpoint is written by `nnUNetTrainer.save_checkpoint` on that object: `.model.pkl` holds the trainer's real class name.

    3-D  base 4, pooling (1,2,2), (2,2,2), kernels (1,3,3), (3,3,3), (3,3,3), patch (6, 24, 20), volume [2, 8, 28, 24]: the reference's own
         SegmentationNetwork.predict_3D(..., regions_class_order=(1, 2, 3), mirror_axes=(0, 1, 2), step_size=0.5, use_gaussian=True) on the
         CPU (pad_nd_image injected from oracle.ops, get_device = "cpu", as make_golden.py does); several tiles in two axes
    2-D  base 8, pooling (2,2), (2,2), (2,1), patch (48, 40), volume [2, 3, 56, 44] (two tiles per axis): the reference's 2-D tiled loop
         cannot run in this snapshot (neural_network.py:718 passes a `normalize` argument :573 does not take); its
         _internal_maybe_mirror_and_pred_2D under the sigmoid does, and tests/_region_refs.predict_3d_2dconv_tiled restates the loop around it

Layout (tests/_region_refs.py puts a folder back together):

    plans_2d.pkl, plans_3d.pkl                           the planners' layouts, 2 modalities
    <2d|3d>/model_final_checkpoint.model[.pkl]            the checkpoint and the trainer's pickle
    <2d|3d>/expected.pt                                   {'raw', 'volume', 'probs', 'seg'}: the seeded case [C,Z,Y,X] as its files hold it, the
                                                          same after the plans' preprocessing (z-score per modality), and the reference's
                                                          probabilities and labels on that
    index.json                                            per dimension: the share of voxels above 0.5 per region (asserted 5-95 %), the share
                                                          of ambiguous voxels (|p - 0.5| <= bar_p) per region and in any region (asserted under
                                                          the tests' 0.5 % cap), the bar, the head seeds

PIN_REPORT_regions.txt lists every file's sha256 and says whether this run reproduced the tree on disk.
"""
import copy
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_refckpt as R  # noqa: E402  (installs the reference import, puts the repository on sys.path)
import make_golden_refckpt3d as R3  # noqa: E402

import _region_refs as RR  # noqa: E402
from cineflow.weights import fill_module_  # noqa: E402
from oracle import ops as OO  # noqa: E402

torch.set_num_threads(8)
TREE = os.path.join(HERE, "ref_model_regions")
TRAINER = "nnUNetTrainerV2BraTSRegions"
ORDER = (1, 2, 3)
DIMS = {
    "2d": dict(threeD=False, base=8, pool=[[2, 2], [2, 2], [2, 1]], kern=[[3, 3]] * 4, patch=(48, 40), volume=(2, 3, 56, 44), task=R.TASK,
               weight_seed=7, input_seed=211),
    "3d": dict(threeD=True, base=4, pool=[[1, 2, 2], [2, 2, 2]], kern=[[1, 3, 3], [3, 3, 3], [3, 3, 3]], patch=(6, 24, 20), volume=(2, 8, 28, 24),
               task=R3.TASK, weight_seed=7, input_seed=213),
}
REPORT = []


def plans_for(dim):
    d = DIMS[dim]
    p = R.reference_plans() if dim == "2d" else R3.reference_plans()
    st = p["plans_per_stage"][0]
    st["patch_size"] = np.array(d["patch"])
    if dim == "2d":
        st["num_pool_per_axis"] = [3, 2]
    st["pool_op_kernel_sizes"], st["conv_kernel_sizes"] = copy.deepcopy(d["pool"]), copy.deepcopy(d["kern"])
    p["base_num_features"] = d["base"]
    p["num_modalities"] = 2
    p["modalities"] = {0: "MRI", 1: "MRI"}
    p["normalization_schemes"] = type(p["normalization_schemes"])([(0, "nonCT"), (1, "nonCT")])
    p["use_mask_for_norm"] = type(p["use_mask_for_norm"])([(0, False), (1, False)])
    ip = p["dataset_properties"]["intensityproperties"]
    ip[1] = copy.deepcopy(ip[0])
    p["dataset_properties"]["modalities"] = {0: "MRI", 1: "MRI"}
    return p


def build_network(cls, dim):
    """the trainer's own initialize_network on an object with the attributes it reads"""
    from nnunet.evaluation.region_based_evaluation import get_brats_regions
    d = DIMS[dim]
    t = cls.__new__(cls)
    t.regions = get_brats_regions()
    t.threeD, t.num_input_channels, t.base_num_features, t.num_classes = d["threeD"], 2, d["base"], len(t.regions)
    t.net_num_pool_op_kernel_sizes, t.net_conv_kernel_sizes, t.conv_per_stage = copy.deepcopy(d["pool"]), copy.deepcopy(d["kern"]), 2
    cls.initialize_network(t)
    assert isinstance(t.network.inference_apply_nonlin, torch.nn.Sigmoid)
    return t.network


def balance_head(net, share_of, lo=0.1, hi=0.9):
    """redraw the rows of the full-resolution head until each region's sliding-window probability is above 0.5 on lo..hi of the voxels
    (share_of(k): that share, from a run of the whole window); returns the seed each row ended with (-1: the filled row stayed)"""
    head = net.seg_outputs[-1].weight
    seeds = []
    for k in range(head.shape[0]):
        seed = -1
        while True:
            if lo <= share_of(k) <= hi:
                break
            seed += 1
            assert seed < 500, "no balanced draw for region channel %d" % k
            with torch.no_grad():
                head[k] = torch.randn(head[k].shape, generator=torch.Generator().manual_seed(1000 * (k + 1) + seed)) * 0.5
        seeds.append(seed)
    return seeds


def sliding_window(net, dim, vol):
    """(probabilities [K,Z,Y,X], labels [Z,Y,X]) of the reference's network on vol [C,Z,Y,X]"""
    from nnunet.network_architecture.neural_network import SegmentationNetwork
    import nnunet.network_architecture.neural_network as nn_mod
    d = DIMS[dim]
    nn_mod.pad_nd_image = OO.pad_nd_image          # batchgenerators is un-vendored: the oracle's restatement, as in make_golden.py
    net.get_device = lambda: "cpu"
    if dim == "3d":
        seg, probs = net.predict_3D(vol, do_mirroring=True, mirror_axes=(0, 1, 2), use_sliding_window=True, step_size=0.5, patch_size=d["patch"],
                                    regions_class_order=ORDER, use_gaussian=True, pad_border_mode="constant", pad_kwargs={"constant_values": 0},
                                    all_in_gpu=False, verbose=False, mixed_precision=False)
        return np.asarray(probs, dtype=np.float32), np.asarray(seg).astype(np.uint8)

    def tile_fn(tile, mult):
        with torch.no_grad():
            return SegmentationNetwork._internal_maybe_mirror_and_pred_2D(net, tile, (0, 1), True, mult)

    probs = RR.predict_3d_2dconv_tiled(tile_fn, net.num_classes, vol, d["patch"], step_size=0.5, use_gaussian=True, pad_border_mode="constant",
                                       pad_kwargs={"constant_values": 0})
    return probs.astype(np.float32), RR.region_labels(probs, ORDER)          # neural_network.py:749-751


def build(out):
    import importlib
    import nnunet.training.network_training.nnUNetTrainer as ref_trainer_mod
    ref_trainer_mod.write_pickle = R.write_pickle
    cls = getattr(importlib.import_module("nnunet.training.network_training.competitions_with_custom_Trainers.BraTS2020." + TRAINER), TRAINER)
    os.makedirs(out)
    index = {"trainer": TRAINER, "regions_class_order": list(ORDER), "bar_p": RR.BAR_P}
    for dim in ("2d", "3d"):
        d = DIMS[dim]
        plans = plans_for(dim)
        R.write_pickle(plans, os.path.join(out, "plans_%s.pkl" % dim))
        net = fill_module_(build_network(cls, dim), d["weight_seed"])
        opt = torch.optim.SGD(net.parameters(), 0.01, weight_decay=3e-5, momentum=0.99, nesterov=True)
        R.one_step(opt, [p for n, p in net.named_parameters() if n.startswith("seg_outputs")])
        net.eval()
        net.do_ds = False
        # the case as its files hold it (one volume per modality) and as the plans' preprocessing hands it to the network: non-CT z-score
        # per modality over the whole volume (preprocessing.py:226-232), no resampling -- the files carry the stage's own spacing
        raw = (R.randn(*d["volume"], seed=d["input_seed"]) * 40 + 100).numpy().astype(np.float32)
        vol = np.stack([((c - c.mean()) / (c.std() + 1e-8)).astype(np.float32) for c in raw])
        seeds = balance_head(net, lambda k: float((sliding_window(net, dim, vol)[0][k] > 0.5).mean()))
        os.makedirs(os.path.join(out, dim))
        R.save_like_the_reference(cls, torch.nn.DataParallel(net), opt, plans, "nnUNet_preprocessed/" + d["task"],
                                  os.path.join(out, dim, "model_final_checkpoint.model"))
        probs, seg = sliding_window(net, dim, vol)
        assert probs.shape == (3,) + d["volume"][1:] and seg.shape == d["volume"][1:] and np.isfinite(probs).all()
        assert np.array_equal(seg, RR.region_labels(probs, ORDER))
        above = [float((probs[k] > 0.5).mean()) for k in range(3)]
        assert all(0.05 <= a <= 0.95 for a in above), (dim, above)
        amb_k = [float((np.abs(probs[k].astype(np.float64) - 0.5) <= RR.BAR_P).mean()) for k in range(3)]
        amb = float(RR.ambiguous(probs).mean())
        assert amb <= RR.AMBIGUOUS_CAP, (dim, amb)
        torch.save({"raw": torch.from_numpy(raw), "volume": torch.from_numpy(vol), "probs": torch.from_numpy(np.ascontiguousarray(probs)),
                    "seg": torch.from_numpy(np.ascontiguousarray(seg))}, os.path.join(out, dim, "expected.pt"))
        index[dim] = {"patch": list(d["patch"]), "volume": list(d["volume"]), "share_above_half": above, "ambiguous_share_per_region": amb_k,
                      "ambiguous_share": amb, "head_seeds": seeds, "labels_present": sorted(int(v) for v in np.unique(seg))}
        REPORT.append("%s %s: head seeds %s; above 0.5 on %s %% of the voxels; |p - 0.5| <= %.2e on %s %% per region, %.4f %% in any; labels %s"
                      % (dim, TRAINER, seeds, ["%.1f" % (100 * a) for a in above], RR.BAR_P, ["%.4f" % (100 * a) for a in amb_k], 100 * amb,
                         index[dim]["labels_present"]))
        print("  " + REPORT[-1])
    with open(os.path.join(out, "index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)


def main():
    before = R.digest(TREE) if os.path.isdir(TREE) else None
    tmp = tempfile.mkdtemp()
    try:
        new = os.path.join(tmp, "ref_model_regions")
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
    with open(os.path.join(HERE, "PIN_REPORT_regions.txt"), "w") as f:
        f.write("tests/golden/ref_model_regions (generated by make_golden_regions.py: the region trainer's own initialize_network, the reference's\n"
                "own save_checkpoint / write_pickle; 3-D outputs by its own predict_3D, 2-D outputs by its own mirror routine inside the\n"
                "restated tile loop of tests/_region_refs.py)\n")
        for line in REPORT:
            f.write(line + "\n")
        for rel in sorted(after):
            f.write("%-62s %8d bytes  sha256 %s\n" % (rel, after[rel][1], after[rel][0]))
        f.write("total %d bytes\n" % sum(n for _h, n in after.values()))
        f.write("rerun: %s\n" % verdict)


if __name__ == "__main__":
    main()
