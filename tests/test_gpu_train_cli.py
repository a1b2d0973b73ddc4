"""python -m cineflow.train end to end at the tiny shape: a four-case stage folder written here (tests/_train_refs.write_stage_folder),
2 epochs x 3 training batches + 2 validation batches on the base-8 network with pools [(2,2),(2,2),(2,1)], patch 40x48, B = 2.

The written model folder loads through cineflow.trainer.load_model_and_checkpoint_files; the inference Generic_UNet with those weights gives
the training forward's full-resolution logits within 1e-4 (the project's logits bar); training_log.txt has one line per epoch; one epoch
followed by -c for the second gives weights bit-identical to the two-epoch run."""
import json
import os

import numpy as np
import pytest
import torch

import _train_refs as R

pytestmark = pytest.mark.gpu


def _train(plans, stage, out, epochs, cont=False):
    from cineflow import train
    argv = ["--plans", plans, "--data", stage, "-o", out, "-f", "0", "--epochs", str(epochs), "--batches_per_epoch", "3", "--val_batches", "2",
            "--seed", "7", "--threads", "4"] + (["-c"] if cont else [])
    train.main(argv)


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("train_cli")
    plans, stage = R.write_stage_folder(root)
    two, split = str(root / "two_epochs"), str(root / "one_plus_one")
    _train(plans, stage, two, 2)
    _train(plans, stage, split, 1)
    _train(plans, stage, split, 2, cont=True)
    return {"plans": plans, "stage": stage, "two": two, "split": split}


def test_model_folder_loads_and_serves_the_trained_weights(runs, dev):
    from cineflow.train_net import TrainNet
    from cineflow.trainer import load_model_and_checkpoint_files
    with open(os.path.join(runs["two"], "plans.json")) as f:
        plans = json.load(f)
    assert plans["mirror_axes"] == [] and "flow_net" not in plans and plans["patch_size"] == [40, 48] and plans["num_classes"] == 4
    trainer, params = load_model_and_checkpoint_files(runs["two"], folds=[0])
    assert len(params) == 1
    trainer.load_checkpoint_ram(params[0], False)
    sd = params[0]["seg_state_dict"]
    init = TrainNet(1, 8, 4, 3, pool_op_kernel_sizes=R.TINY_POOL).to(dev).init_weights(7).state_dict()
    moved = [k for k in sd if not torch.equal(sd[k], init[k])]
    assert "seg_outputs.0.weight" not in moved and len(moved) == len(sd) - 1, "every tensor but the unsupervised head has been trained"
    x = torch.randn(2, 1, 40, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    want = TrainNet(1, 8, 4, 3, pool_op_kernel_sizes=R.TINY_POOL).load_state_dict(sd, dev).forward_train(x)[0]
    got = trainer.seg_net(x)
    err = float((got - want).abs().max())
    print("inference Generic_UNet vs training forward: max |dlogit| %.3e" % err)
    assert got.shape == want.shape and err <= 1e-4


def test_training_log_has_one_line_per_epoch(runs):
    lines = open(os.path.join(runs["two"], "fold_0", "training_log.txt")).read().strip().split("\n")
    assert len(lines) == 2
    for i, l in enumerate(lines):
        f = l.split()
        assert f[:2] == ["epoch", str(i)] and f[2] == "lr" and f[4] == "train_loss" and f[6] == "val_loss" and f[8] == "mean_fg_dice"
        assert all(np.isfinite(float(f[j])) for j in (3, 5, 7, 9))
    assert float(lines[0].split()[3]) == 1e-2 and float(lines[1].split()[3]) == pytest.approx(1e-2 * 0.5 ** 0.9, rel=1e-5)


def test_continue_gives_the_same_bits(runs):
    a = torch.load(os.path.join(runs["two"], "fold_0", "model_final_checkpoint.model"), weights_only=True)["seg_state_dict"]
    b = torch.load(os.path.join(runs["split"], "fold_0", "model_final_checkpoint.model"), weights_only=True)["seg_state_dict"]
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    la = open(os.path.join(runs["two"], "fold_0", "training_log.txt")).read().strip().split("\n")
    lb = open(os.path.join(runs["split"], "fold_0", "training_log.txt")).read().strip().split("\n")
    assert la[1] == lb[1] and len(lb) == 2
