"""Yardstick of the training tests (test_gpu_train_ops.py, test_gpu_train_step.py, test_gpu_train_cli.py).

The truth is fp64 torch autograd on the CPU.  The bar is not a fixed number: the same computation in fp32 torch on the CPU is run next to it,
its error against fp64 is measured by `rel_err`, and the device may have at most FACTOR x that error, with a floor of FLOOR.  The device sums
the same fp32 terms in another order and partition, which moves the error by a small factor; a missing tap, a wrong stride or a dropped
split gives 1e-2 or more.

Metric per tensor: |g - g64|_2 / max(|g64|_2, 1e-3 |all gradients|_2) -- the second term keeps tensors whose true gradient is zero
(a convolution bias under an InstanceNorm) meaningful."""
import numpy as np
import torch
import torch.nn.functional as F

FACTOR = 4.0
FLOOR = 1e-6


def leaf(t, dtype):
    """a fresh leaf of that dtype (t.to(dtype) alone returns t itself when the dtype already matches)"""
    return t.detach().to(dtype).clone().requires_grad_(True)


def total_norm(tensors):
    return float(torch.sqrt(sum((t.double() ** 2).sum() for t in tensors)))


def rel_err(g, g64, all_norm):
    return float((g.double() - g64).norm()) / max(float(g64.norm()), 1e-3 * all_norm)


def hold(name, dev_t, cpu32, ref64, all_norm):
    """print the figures, then assert the device error <= max(FACTOR x the fp32 CPU error, FLOOR)"""
    e32 = rel_err(cpu32, ref64, all_norm)
    ed = rel_err(dev_t.detach().cpu(), ref64, all_norm)
    bar = max(FACTOR * e32, FLOOR)
    print("%-56s cpu32 %.3e  device %.3e  bar %.3e" % (name, e32, ed, bar))
    assert ed <= bar, (name, ed, bar)
    return ed


def hold_scalar(name, dev_v, cpu32_v, ref64_v):
    e32 = abs(float(cpu32_v) - float(ref64_v)) / max(abs(float(ref64_v)), 1e-3)
    ed = abs(float(dev_v) - float(ref64_v)) / max(abs(float(ref64_v)), 1e-3)
    bar = max(FACTOR * e32, FLOOR)
    print("%-56s cpu32 %.3e  device %.3e  bar %.3e" % (name, e32, ed, bar))
    assert ed <= bar, (name, ed, bar)


# ---- the loss, restated in torch (loss_functions/dice_loss.py:101-154,201-237,436-497; deep_supervision.py) -------------------------------
def dc_ce_loss(logits, target, smooth=1e-5):
    """DC_and_CE_loss({'batch_dice': True, 'smooth': 1e-5, 'do_bg': False}, {}) of this fork: CE + (1 - mean dice over classes 1..)"""
    K = logits.shape[1]
    p = torch.softmax(logits, 1)
    y = F.one_hot(target.long(), K).permute(0, 3, 1, 2).to(logits.dtype)
    axes = (0, 2, 3)
    tp = (p * y).sum(axes)
    fp = (p * (1 - y)).sum(axes)
    fn = ((1 - p) * y).sum(axes)
    dc = (2 * tp + smooth) / (2 * tp + fp + fn + smooth + 1e-8)
    return F.cross_entropy(logits, target.long()) + 1 - dc[1:].mean()


def multiple_output_loss(outputs, targets, weights):
    """MultipleOutputLoss2: a zero-weight output is skipped entirely"""
    l = weights[0] * dc_ce_loss(outputs[0], targets[0])
    for i in range(1, len(outputs)):
        if weights[i] != 0:
            l = l + weights[i] * dc_ce_loss(outputs[i], targets[i])
    return l


# ---- the network: oracle.models.GenericUNet2D with deep supervision on --------------------------------------------------------------------
def forward_heads(net, x):
    """GenericUNet2D.forward, but returning every head: full resolution first, then each coarser decoder stage (generic_UNet.py:389-408
    with _deep_supervision and do_ds on; upscale_logits off)."""
    skips, seg = [], []
    for d in range(len(net.conv_blocks_context) - 1):
        x = net.conv_blocks_context[d](x)
        skips.append(x)
    x = net.conv_blocks_context[-1](x)
    for u in range(len(net.tu)):
        x = net.tu[u](x)
        x = torch.cat((x, skips[-(u + 1)]), dim=1)
        x = net.conv_blocks_localization[u](x)
        seg.append(net.seg_outputs[u](x))
    return [seg[-1]] + seg[:-1][::-1]


def ring_labels(B, H, W, K):
    """concentric rings around a centre that moves with the sample: every class present in every sample"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((B, H, W), np.int64)
    for b in range(B):
        r = np.sqrt((yy - H / 2 - b) ** 2 + (xx - W / 2 + 2 * b) ** 2) / (min(H, W) / 2)
        out[b] = np.clip((K - 1) - np.floor(r * K).astype(np.int64), 0, K - 1)
    return out


def downsample_targets(labels, scales):
    """DownsampleSegForDSTransform2 at order 0 through the project's restatement, cineflow.preprocessing.resize_segmentation"""
    from cineflow.preprocessing import resize_segmentation
    out = []
    for s in scales:
        if all(v == 1 for v in s):
            out.append(labels.copy())
            continue
        shp = np.round(np.array(labels.shape[1:]) * np.array(s)).astype(int)
        out.append(np.stack([resize_segmentation(labels[b], shp, order=0) for b in range(labels.shape[0])]).astype(labels.dtype))
    return out


# ---- a tiny preprocessed task: stage folder (<case>.npz data + seg, <case>.pkl with class_locations) and the plans pickle ------------------
TINY_POOL = [[2, 2], [2, 2], [2, 1]]
TINY_PATCH = [40, 48]


def write_stage_folder(root, batch_size=2, shapes=((3, 44, 52), (2, 40, 48), (3, 36, 40), (4, 50, 60))):
    """-> (plans pickle, stage folder).  Case 2 is smaller than the patch on both axes (padding), case 3 larger (a real random crop)."""
    import os
    import pickle
    stage = os.path.join(str(root), "task", "nnUNetData_plans_v2.1_2D_stage0")
    os.makedirs(stage)
    rs = np.random.RandomState(5)
    for i, (D, H, W) in enumerate(shapes):
        seg = ring_labels(D, H, W, 4).astype(np.float32)
        img = (seg + 0.3 * rs.randn(D, H, W)).astype(np.float32)
        np.savez(os.path.join(stage, "case_%03d.npz" % i), data=np.stack([img, seg]))
        loc = {c: np.argwhere(seg == c) for c in (1, 2, 3)}
        with open(os.path.join(stage, "case_%03d.pkl" % i), "wb") as f:
            pickle.dump({"class_locations": loc, "classes": np.array([0, 1, 2, 3])}, f)
    plans = {"num_modalities": 1, "num_classes": 3, "base_num_features": 8, "conv_per_stage": 2, "transpose_forward": [0, 1, 2],
             "transpose_backward": [0, 1, 2], "normalization_schemes": {0: "nonCT"}, "use_mask_for_norm": {0: False},
             "dataset_properties": {"intensityproperties": None}, "preprocessor_name": "PreprocessorFor2D",
             "plans_per_stage": {0: {"batch_size": batch_size, "patch_size": np.array(TINY_PATCH), "pool_op_kernel_sizes": TINY_POOL,
                                     "conv_kernel_sizes": [[3, 3]] * 4, "num_pool_per_axis": [3, 2]}}}
    plans_file = os.path.join(str(root), "task", "nnUNetPlansv2.1_plans_2D.pkl")
    with open(plans_file, "wb") as f:
        pickle.dump(plans, f)
    names = ["case_%03d" % i for i in range(len(shapes))]                 # four cases are too few for the five-fold split: one split, given
    with open(os.path.join(str(root), "task", "splits_final.pkl"), "wb") as f:
        pickle.dump([{"train": names[:-1], "val": names[-1:]}], f)
    return plans_file, stage
