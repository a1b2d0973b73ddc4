"""One and three training iterations of cineflow.train_net.TrainNet + the train_ops loss and optimizer, on the network of
tests/golden/make_golden_train.py: base 8, 3 pools [(2,2),(2,2),(2,1)], patch 40x48, B = 2, K = 4, one input channel (bottleneck 5x12), ring
labels (every class present), the reference's initial weights.

  one step     loss and every gradient against fp64 autograd of oracle.models.GenericUNet2D (all heads: _train_refs.forward_heads) on the
               CPU, by the yardstick of tests/_train_refs.py; seg_outputs.0.weight has no gradient
  three steps  parameters against the golden trajectory written by the reference's Generic_UNet, loss, clipping and SGD in fp64, the fp32
               CPU run of the same three steps (oracle network) setting the bar; seg_outputs.0.weight bit-identical to its initial value
  repeat       the whole step from the same state gives the same bits

Figures measured on an MI355X (max over tensors; the bar is 4 x the fp32 CPU figure, floor 1e-6) are kept in profiles/train_step.md."""
import numpy as np
import pytest
import torch

import _train_refs as R

pytestmark = pytest.mark.gpu

POOL = [(2, 2), (2, 2), (2, 1)]
WEIGHTS = [2 / 3, 1 / 3, 0.0]
NOGRAD = "seg_outputs.0.weight"


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("train/step")
    init = {k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init/")}
    return {"x": torch.from_numpy(g["x"]), "labels": g["labels"], "targets": [g["target%d" % i] for i in range(3)], "init": init,
            "losses": g["losses"], "scales": g["scales"], "final": {k: torch.from_numpy(v) for k, v in golden("train/step_final").items()}}


def _oracle(fx, dtype):
    from oracle import models as OM
    net = OM.GenericUNet2D(1, 8, 4, 3, pool_op_kernel_sizes=POOL).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in fx["init"].items()}, strict=True)
    return net.train()


def _cpu_steps(fx, dtype, n):
    """n iterations of run_iteration's fp32 branch on the oracle network -> (losses, gradients of the LAST backward before clipping, net)"""
    net = _oracle(fx, dtype)
    opt = torch.optim.SGD(net.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    tg = [torch.from_numpy(t) for t in fx["targets"]]
    losses, grads = [], None
    for _ in range(n):
        opt.zero_grad()
        l = R.multiple_output_loss(R.forward_heads(net, fx["x"].to(dtype)), tg, WEIGHTS)
        l.backward()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}
        torch.nn.utils.clip_grad_norm_(net.parameters(), 12)
        opt.step()
        losses.append(l.detach())
    return losses, grads, net


@pytest.fixture(scope="module")
def cpu(fx):
    return {(dt, n): _cpu_steps(fx, dt, n) for dt in (torch.float64, torch.float32) for n in (1, 3)}


def _device_net(fx, dev):
    from cineflow.train_net import TrainNet
    return TrainNet(1, 8, 4, 3, pool_op_kernel_sizes=POOL).load_state_dict(fx["init"], dev)


def _device_step(net, fx, dev, first, targets=None):
    from cineflow import train_ops as T
    tg = targets or [torch.from_numpy(t).to(torch.int32).to(dev) for t in fx["targets"]]
    outs = net.forward_train(fx["x"].to(dev))
    loss, dl = T.deep_supervision_loss(outs, tg, WEIGHTS)
    no_grad = net.backward(dl)
    table = net.table(no_grad)
    nc = T.grad_norm(net.grad, table, len(net.names))
    grads = net.grad_dict()
    T.sgd_nesterov(net.param, net.grad, net.mom, table, len(net.names), net.max_tensor, nc, 1e-2, 3e-5, 0.99, first=first)
    return loss, no_grad, grads, outs


def test_targets_are_the_reference_downsampling(fx, dev):
    """DownsampleSegForDSTransform2 at order 0 == cineflow.preprocessing.resize_segmentation (the sampling point is not [::2])"""
    got = R.downsample_targets(fx["labels"], [list(s) for s in fx["scales"]])
    for i, (a, b) in enumerate(zip(got, fx["targets"])):
        assert a.shape == b.shape and np.array_equal(a, b), i
    assert not np.array_equal(fx["targets"][1], fx["labels"][:, ::2, ::2])


def test_golden_trajectory_agrees_with_the_oracle(fx, cpu):
    """the reference's three fp64 losses and final weights == the oracle network under the restated loss (the CPU yardstick is sound)"""
    losses, _g, net = cpu[(torch.float64, 3)]
    assert np.allclose([float(l) for l in losses], fx["losses"], rtol=1e-12, atol=0)
    for k, v in net.state_dict().items():
        assert float((v - fx["final"][k]).abs().max()) <= 1e-12, k


def test_one_step_loss_and_gradients(fx, cpu, dev):
    net = _device_net(fx, dev)
    loss, no_grad, grads, outs = _device_step(net, fx, dev, True)
    assert no_grad == {NOGRAD}
    l64, g64, _ = cpu[(torch.float64, 1)]
    l32, g32, _ = cpu[(torch.float32, 1)]
    assert g64[NOGRAD] is None
    R.hold_scalar("loss", loss.item(), l32[0], l64[0])
    names = [k for k in net.names if k != NOGRAD]
    alln = R.total_norm([g64[k] for k in names])
    worst = max(R.hold(k, grads[k], g32[k], g64[k], alln) for k in names)
    print("worst device gradient error %.3e" % worst)


def test_three_steps_parameters(fx, cpu, dev):
    net = _device_net(fx, dev)
    losses = [_device_step(net, fx, dev, i == 0)[0].item() for i in range(3)]
    l32, _g, net32 = cpu[(torch.float32, 3)]
    for i in range(3):
        R.hold_scalar("loss of step %d" % i, losses[i], l32[i], fx["losses"][i])
    sd, sd32 = net.state_dict(), net32.state_dict()
    assert torch.equal(sd[NOGRAD], fx["init"][NOGRAD]), "a head without a gradient leaves training bit-identical: no step, no weight decay"
    alln = R.total_norm(list(fx["final"].values()))
    for k in net.names:
        R.hold("param " + k, sd[k], sd32[k], fx["final"][k], alln)


def test_step_is_bit_reproducible(fx, dev):
    a, b = _device_net(fx, dev), _device_net(fx, dev)
    ra, rb = _device_step(a, fx, dev, True), _device_step(b, fx, dev, True)
    assert torch.equal(ra[0], rb[0])
    for k in a.names:
        assert torch.equal(ra[2][k], rb[2][k]), k
    assert torch.equal(a.param, b.param) and torch.equal(a.mom, b.mom)
    for oa, ob in zip(ra[3], rb[3]):
        assert torch.equal(oa, ob)
