#!/usr/bin/env python3
"""Time one training step of cineflow.train_net at the ACDC 2-D plan shape -- patch 256x224, base 32, pools [[2,2]]*5 + [[2,1]], the batch
size the 2-D planner's memory estimate gives that patch -- and the same step of oracle.models.GenericUNet2D under torch autograd in fp32 on
the same device (how a user of the reference trains today).

    python tools/train_bench.py [--steps 5] [--warmup 2] [--batch N] [--out profiles/train_step.md] [--no-torch]

Step time: host clock around a step that ends in a device synchronise, median of the steps after warm-up.  The split between forward,
loss, backward and optimizer comes from device events recorded between the phases of the same steps.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PATCH, BASE, K = (256, 224), 32, 4
POOL = [[2, 2]] * 5 + [[2, 1]]


def plan_batch_size():
    from cineflow.experiment_planning import Generic_UNet as G
    est = G.compute_approx_vram_consumption(PATCH, [6, 5], BASE, 512, 1, K, POOL, conv_per_stage=2)
    return int(np.floor(G.use_this_for_batch_size_computation_2D / est * G.DEFAULT_BATCH_SIZE_2D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench needs a GPU"
    import _train_refs as R
    from cineflow import train_ops as T
    from cineflow.train_net import TrainNet, deep_supervision_scales, deep_supervision_weights
    from oracle import models as OM
    dev = torch.device("cuda:0")
    B = a.batch or plan_batch_size()
    weights = [float(w) for w in deep_supervision_weights(len(POOL))]
    scales = deep_supervision_scales(POOL)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, 1, *PATCH, generator=gen).to(dev)
    labels = R.ring_labels(B, PATCH[0], PATCH[1], K)
    targets = [torch.from_numpy(t).to(torch.int32).to(dev).contiguous() for t in R.downsample_targets(labels, scales)]

    net = TrainNet(1, BASE, K, len(POOL), pool_op_kernel_sizes=POOL).to(dev).init_weights(3)
    sd = net.state_dict()
    phases = ("forward", "loss", "backward", "optimizer")
    split = {p: [] for p in phases}
    times, losses = [], []
    for it in range(a.warmup + a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        outs = net.forward_train(x)
        ev[1].record()
        loss, dl = T.deep_supervision_loss(outs, targets, weights)
        ev[2].record()
        no_grad = net.backward(dl)
        ev[3].record()
        table = net.table(no_grad)
        clip = T.grad_norm(net.grad, table, len(net.names))
        T.sgd_nesterov(net.param, net.grad, net.mom, table, len(net.names), net.max_tensor, clip, 1e-2, first=it == 0)
        ev[4].record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        losses.append(float(loss))
        if it >= a.warmup:
            times.append(dt)
            for i, p in enumerate(phases):
                split[p].append(ev[i].elapsed_time(ev[i + 1]) * 1e-3)
    ours = statistics.median(times)
    lines = ["batch %d, patch %dx%d, base %d, pools %s, %d timed steps after %d warm-up" % (B, PATCH[0], PATCH[1], BASE, POOL, a.steps, a.warmup),
             "cineflow step: median %.4f s (min %.4f, max %.4f); losses %s" % (ours, min(times), max(times), ["%.4f" % l for l in losses]),
             "  split (median device seconds): " + ", ".join("%s %.4f" % (p, statistics.median(split[p])) for p in phases)]
    del outs, dl
    if not a.no_torch:
        try:
            ref = OM.GenericUNet2D(1, BASE, K, len(POOL), pool_op_kernel_sizes=POOL)
            ref.load_state_dict(sd, strict=True)
            ref = ref.to(dev).train()
            opt = torch.optim.SGD(ref.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
            tl = [t.long() for t in targets]
            rt, rl = [], []
            for it in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.zero_grad()
                l = R.multiple_output_loss(R.forward_heads(ref, x), tl, weights)
                l.backward()
                torch.nn.utils.clip_grad_norm_(ref.parameters(), 12)
                opt.step()
                torch.cuda.synchronize()
                rl.append(float(l))
                if it >= a.warmup:
                    rt.append(time.perf_counter() - t0)
            theirs = statistics.median(rt)
            lines.append("torch autograd fp32 step (oracle GenericUNet2D, same device): median %.4f s (min %.4f, max %.4f); losses %s"
                         % (theirs, min(rt), max(rt), ["%.4f" % l for l in rl]))
            lines.append("ratio cineflow / torch = %.2f" % (ours / theirs))
        except RuntimeError as e:
            lines.append("torch autograd reference did not run on this machine: %s" % str(e).split("\n")[0])
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
