"""tests/golden/ref_model_variants (make_golden_variants.py) as the reference's trainer variants wrote it: `folder` puts one trainer's
model folder back together -- plans.pkl, fold_0/model_final_checkpoint.model (stored once per distinct file under models/) and the
trainer's own .model.pkl -- and `expected` gives the seeded input and the reference network's logits."""
import json
import os
import shutil

import torch

TREE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_model_variants")
BAR = 1e-4            # the logits bar tests/test_gpu_models.py applies to the reduced-width Generic_UNet / generic_unet_3d fixtures
CHK = "model_final_checkpoint"

with open(os.path.join(TREE, "index.json")) as _f:
    INDEX = json.load(_f)
CASES = [(dim, name) for dim in ("2d", "3d") for name in sorted(INDEX[dim])]


def folder(dim, name, dst):
    """the trainer's output folder at `dst` (created); returns dst"""
    row = INDEX[dim][name]
    os.makedirs(os.path.join(dst, "fold_0"))
    shutil.copy(os.path.join(TREE, row["plans"]), os.path.join(dst, "plans.pkl"))
    shutil.copy(os.path.join(TREE, "models", row["model"]), os.path.join(dst, "fold_0", CHK + ".model"))
    shutil.copy(os.path.join(TREE, dim, name, CHK + ".model.pkl"), os.path.join(dst, "fold_0", CHK + ".model.pkl"))
    return dst


def expected(dim, name):
    """(x, logits): the seeded input of the dimension and the reference network's fp32 logits on it"""
    x = torch.load(os.path.join(TREE, "inputs.pt"), map_location="cpu", weights_only=True)[dim]
    return x, torch.load(os.path.join(TREE, dim, name, "logits.pt"), map_location="cpu", weights_only=True)["logits"]


def near_tie(values, bar, dim=1):
    """bool mask: the top two entries along `dim` lie within `bar` of each other"""
    top = torch.topk(values.double(), 2, dim=dim).values
    return (top.select(dim, 0) - top.select(dim, 1)) <= bar
