#!/usr/bin/env python3
"""Generate tests/golden/train/*.npz by RUNNING THE REFERENCE'S training classes on the CPU (no source of theirs is copied; their outputs are
data).

    python tests/golden/make_golden_train.py

  train/loss.npz    MultipleOutputLoss2(DC_and_CE_loss({'batch_dice': True, 'smooth': 1e-5, 'do_bg': False}, {}), (2/3, 1/3, 0)) on seeded
                    logits (K = 4, B = 2, 8x12 and two coarser outputs): loss and dlogits in fp64 and in fp32
  train/step.npz    Generic_UNet(1, 8, 4, 3 pools [(2,2),(2,2),(2,1)], deep supervision on), InitWeights_He(1e-2), patch 40x48, B = 2, ring
                    labels; targets by downsample_seg_for_ds_transform2 at order 0; three iterations of nnUNetTrainerV2.run_iteration's fp32
                    branch restated around the reference's network and loss -- loss, backward, clip_grad_norm_(12), SGD(1e-2, wd 3e-5,
                    momentum 0.99, nesterov) -- in fp64: input, labels, targets, initial weights (fp32 values), three losses
  train/step_final.npz   the weights after those three iterations (fp64)

skimage and batchgenerators are absent from the build image: the reference's downsampling module gets oracle.preprocess.resize_segmentation
injected for batchgenerators' function of that name, as tests/golden/make_golden.py does for the preprocessing pins (parity of that one
function unpinned)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "cardiac-segmentation-optical-flow_amd"))

import _ref_import  # noqa: E402

OUT = os.path.join(HERE, "train")
WEIGHTS = (2 / 3, 1 / 3, 0.0)
POOL = [[2, 2], [2, 2], [2, 1]]


def main():
    _ref_import.install()
    from nnunet.network_architecture.generic_UNet import Generic_UNet
    from nnunet.network_architecture.initialization import InitWeights_He
    from nnunet.training.loss_functions.dice_loss import DC_and_CE_loss
    from nnunet.training.loss_functions.deep_supervision import MultipleOutputLoss2
    from nnunet.training.data_augmentation import downsampling
    from oracle import preprocess as OP
    import _train_refs as R
    downsampling.resize_segmentation = OP.resize_segmentation
    os.makedirs(OUT, exist_ok=True)

    def ref_loss():
        return MultipleOutputLoss2(DC_and_CE_loss({"batch_dice": True, "smooth": 1e-5, "do_bg": False}, {}), WEIGHTS)

    # ---------------------------------------------------------------------------------------------- loss
    gen = torch.Generator().manual_seed(101)
    B, K, H, W = 2, 4, 8, 12
    shapes = [(H, W), (H // 2, W // 2), (H // 4, W // 4)]
    logits = [(torch.randn(B, K, *s, generator=gen) * 2) for s in shapes]
    targets = [torch.randint(0, K, (B, 1) + s, generator=gen) for s in shapes]
    arrays = {"n_outputs": np.int64(3), "weights": np.array(WEIGHTS)}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ls = [R.leaf(l, dt) for l in logits]
        loss = ref_loss()(ls, [t.to(dt) for t in targets])
        loss.backward()
        arrays["loss" + tag] = loss.detach().numpy()
        for i, l in enumerate(ls):
            if l.grad is not None:
                arrays["grad%s_%d" % (tag, i)] = l.grad.numpy()
        assert ls[2].grad is None
    for i in range(3):
        arrays["logits%d" % i] = logits[i].numpy()
        arrays["target%d" % i] = targets[i][:, 0].numpy().astype(np.int32)
    restated = R.multiple_output_loss([l.double() for l in logits], [t[:, 0] for t in targets], WEIGHTS)
    print("loss: reference fp64 %.12f, fp32 %.9f, tests/_train_refs.py restatement %.12f" % (arrays["loss64"], arrays["loss32"], restated))
    np.savez_compressed(os.path.join(OUT, "loss.npz"), **arrays)

    # ---------------------------------------------------------------------------------------------- three training iterations
    torch.manual_seed(202)
    net = Generic_UNet(1, 8, 4, 3, 2, 2, torch.nn.Conv2d, torch.nn.InstanceNorm2d, {"eps": 1e-5, "affine": True}, torch.nn.Dropout2d,
                       {"p": 0, "inplace": True}, torch.nn.LeakyReLU, {"negative_slope": 1e-2, "inplace": True}, True, False, lambda x: x,
                       InitWeights_He(1e-2), POOL, [[3, 3]] * 4, False, True, True)
    net.train()
    net.do_ds = True
    init = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    net = net.double()
    B, H, W = 2, 40, 48
    x = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(203))
    labels = R.ring_labels(B, H, W, 4)
    scales = [[1, 1]] + [list(v) for v in 1 / np.cumprod(np.vstack(POOL), axis=0)][:-1]          # nnUNetTrainerV2.py:111-112
    tgts = downsampling.downsample_seg_for_ds_transform2(labels[:, None].astype(np.float32), scales, 0, None)
    opt = torch.optim.SGD(net.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    loss_fn = ref_loss()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = net(x.double())
        assert len(out) == 3 and [tuple(o.shape[2:]) for o in out] == [tuple(t.shape[2:]) for t in tgts]
        l = loss_fn(out, [torch.from_numpy(t).double() for t in tgts])
        l.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 12)
        opt.step()
        losses.append(float(l))
    assert net.seg_outputs[0].weight.grad is None
    print("three losses:", losses)
    arrays = {"x": x.numpy(), "labels": labels.astype(np.int32), "losses": np.array(losses), "scales": np.array(scales, dtype=np.float64)}
    for i, t in enumerate(tgts):
        arrays["target%d" % i] = t[:, 0].astype(np.int32)
    for k, v in init.items():
        arrays["init/" + k] = v
    np.savez_compressed(os.path.join(OUT, "step.npz"), **arrays)
    np.savez_compressed(os.path.join(OUT, "step_final.npz"), **{k: v.detach().numpy() for k, v in net.state_dict().items()})
    for f in ("loss.npz", "step.npz", "step_final.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
