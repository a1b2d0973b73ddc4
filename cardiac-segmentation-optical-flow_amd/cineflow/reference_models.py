"""Import of the model folders the reference's trainers write, into the `plans.json` + `fold_X/<chk>.model` format of cineflow.predict.

The reference trains its two networks separately and writes

    <seg_folder>/plans.pkl                              nnU-Net 2-D plans (predict.py:691-694)
    <seg_folder>/fold_X/<chk>.model                     torch.save({epoch, state_dict, optimizer_state_dict, lr_scheduler_state_dict,
                                                        plot_stuff, best_stuff[, amp_grad_scaler]})  (network_trainer.py:305-335)
    <seg_folder>/fold_X/<chk>.model.pkl                 {init, name, class (a str), plans}  (nnUNetTrainer.py:4302-4310)
    <flow_weights>/config.yaml                          the flow network's YAML (run_training.py:191)
    <flow_weights>/<task>/fold_X/<chk>.model[.pkl]      the flow trainer's checkpoint (run_training.py:283)

`import_reference_model_folder` pairs one segmentation folder with one flow folder and writes a folder that `predict_from_folder(model=...)`
and `python -m cineflow.predict -m ...` take unchanged (save_model_folder).  Nothing here imports or calls a global named by a file:
`.pkl` files go through a restricted unpickler (cineflow.safe_pickle, widened only by plain-data globals), `.model` files through
`torch.load(weights_only=True)` with numpy's scalar / array / dtype reconstructors admitted (the losses in `plot_stuff` / `best_stuff` are
`np.mean(...)` results, which plain `weights_only=True` refuses).  Every tensor is checked against the networks the new plans build before
anything is written.  Values the build cannot honour raise `NotImplementedError` naming the key, as cineflow.config does.

Without a flow folder (`import_reference_model_folder(seg_folder, None, out)`, no `-w`) an nnU-Net folder is imported on its own: the
plans get no 'flow_net', the checkpoints no 'flow_state_dict', and predict_from_folder takes the segmentation-only route.  The stage's
patch length picks the translation: 2 entries -> plans_from_reference (Generic_UNet), 3 entries -> plans_from_reference_3d (a `3d_fullres`
folder, Generic_UNet3D on the native 3-D convolution).  A 3-D folder paired with a flow folder is refused: the flow path is 2-D.
A `3d_cascade_fullres` folder -- recognised by its trainer's name or by a first convolution that is num_classes input channels wider than
the modalities -- gets seg_net.prev_stage_classes = [1 .. num_classes]: the previous stage's labels become input channels
(predict_from_folder's lowres_segmentations / -l).  Its `3d_lowres` sibling is an ordinary 3-D folder of stage 0 of the same plans.
A folder of nnUNetTrainerV2_ResencUNet (or its _DA3 variant) -- recognised by num_blocks_encoder in the stage, cross-checked against the
trainer's name -- gets seg_net.arch = 'resenc': the residual-encoder U-Net (FabiansUNet3D).  The decoder tensors the reference registers
twice are checked for equality and kept once.  Its BatchNorm variants (_BN trainers, running statistics in the checkpoint) are refused.

A folder of nnMTLTrainerV2 -- recognised by its trainer's name -- is imported with `--seg_config` (the trainer's YAML) and without `-w` as a
seg_net.arch = 'mtl' folder: the fork's own MTLmodel segmenter, behind the 2-class MTLmodel cropper when the YAML sets `cropper: true`
(`--crop_weights`, `--crop_config` are then required).

Command line:  python -m cineflow.reference_models -s SEG [-w FLOW] -o OUT [--seg_config Y] [--crop_weights F --crop_config Y] [-f FOLDS] [-chk NAME] [--seg_variant NAME]
               [--seg_regions NAME_OR_JSON] [--seg_regions_class_order L [L ...]]
"""
import argparse
import os
import re
import shutil

import numpy as np
import torch

from .safe_pickle import PlainUnpickler, load_plain_pickle
from .trainer import CineTrainer, save_model_folder

join = os.path.join

_DROPPED_CHECKPOINT_KEYS = ("optimizer_state_dict", "lr_scheduler_state_dict", "amp_grad_scaler")
# buffers the networks rebuild from their constructor arguments and never load: SpatialTransformer grids (trainer._broadcast_params),
# BatchNorm step counters, Swin relative-position indices and shift masks (the MTLmodel cropper's state_dict holds all three)
_DERIVED_BUFFERS = ("grid", "num_batches_tracked", "relative_position_index", "attn_mask")


# ------------------------------------------------------------------------------------------------ safe readers
class ReferencePickleUnpickler(PlainUnpickler):
    """PlainUnpickler plus the plain-data globals nnU-Net's `plans.pkl` / `<chk>.model.pkl` need: `set` / `frozenset` (a GLOBAL under
    pickle protocols <= 3, `__builtin__` under protocol 2) and numpy's dtype classes."""

    _ALLOWED = PlainUnpickler._ALLOWED | {
        ("builtins", "set"), ("builtins", "frozenset"), ("__builtin__", "set"), ("__builtin__", "frozenset"),
    } | {("numpy.dtypes", type(np.dtype(c)).__name__) for c in "?bBhHiIlLqQefdg"}
    _WHAT = "a reference pickle"


def load_reference_pickle(path):
    """`plans.pkl` / `<chk>.model.pkl` -> plain Python / numpy values; any other global raises pickle.UnpicklingError."""
    return load_plain_pickle(path, ReferencePickleUnpickler)


def _numpy_safe_globals():
    """numpy's scalar / array reconstructors and the dtype classes torch's weights-only unpickler must be told about"""
    try:
        from numpy._core import multiarray as ma
    except ImportError:                                                       # numpy < 2
        from numpy.core import multiarray as ma
    dtypes = sorted({type(np.dtype(c)) for c in "?bBhHiIlLqQefdg"}, key=lambda t: t.__name__)
    return [ma.scalar, ma._reconstruct, np.ndarray, np.dtype] + [t for t in dtypes if t is not np.dtype]


def strip_module_prefix(state_dict, expected=None):
    """network_trainer.py:418-440: a key that the network does not have and that starts with `module.` (nn.DataParallel) loses the prefix.
    Without `expected` every `module.` prefix is dropped."""
    out = {}
    for k, v in state_dict.items():
        if k.startswith("module.") and (expected is None or k not in expected):
            k = k[len("module."):]
        out[k] = v
    return out


def load_reference_checkpoint(path, expected=None):
    """`<chk>.model` of a reference trainer -> the checkpoint dict without its optimizer / scheduler / grad-scaler entries, `state_dict`
    with the `module.` prefix stripped (`expected`: the network's key names, for the reference's exact rule).  torch.load runs with
    weights_only=True; numpy's scalar / array / dtype reconstructors are the only globals added."""
    with torch.serialization.safe_globals(_numpy_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "state_dict" not in ck:
        raise KeyError("%s holds no 'state_dict' entry (not a checkpoint written by NetworkTrainer.save_checkpoint)" % path)
    out = {k: v for k, v in ck.items() if k not in _DROPPED_CHECKPOINT_KEYS}
    out["state_dict"] = strip_module_prefix(ck["state_dict"], expected)
    return out


# ------------------------------------------------------------------------------------------------ plans
def _plain(obj):
    """numpy values / tuples / sets / non-string keys -> what json.dump writes"""
    if isinstance(obj, dict):
        return {str(_plain(k)) if not isinstance(k, str) else k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    if isinstance(obj, (set, frozenset)):
        return sorted(_plain(v) for v in obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def _refuse(key, value, built):
    raise NotImplementedError("plans_from_reference: %s = %r is outside what the build implements (built: %s)" % (key, value, built))


def plans_from_reference(plans, stage=None):
    """The reference's 2-D nnU-Net plans (experiment_planner_baseline_2DUNet.py:148-160) -> the plans dict CineTrainer reads.

    The stage is chosen as nnUNetTrainer.py:478-482 does (None: the plans must have exactly one); the segmentation network is the
    Generic_UNet nnUNetTrainerV2.py:147-169 builds from it (num_classes + 1 outputs, one pooling stage per pool_op_kernel_sizes entry,
    3x3 convolutions, conv_per_stage 2).  crop_size / image_size / flow_net are the flow trainer's and are added by the importer."""
    stages = plans["plans_per_stage"]
    if stage is None:
        if len(stages) != 1:
            raise ValueError("plans_from_reference: the plans have %d stages %s; pass stage= (nnUNetTrainer.py:479-481)" % (len(stages), sorted(stages)))
        stage = list(stages.keys())[0]
    if stage not in stages:
        raise KeyError("plans_from_reference: stage %r is not in plans_per_stage %s" % (stage, sorted(stages)))
    sp = stages[stage]
    patch = [int(v) for v in np.asarray(sp["patch_size"]).ravel()]
    if len(patch) != 2:
        _refuse("plans_per_stage[%r]['patch_size']" % stage, patch, "2-D stages")
    if "pool_op_kernel_sizes" in sp:
        pool = [[int(v) for v in p_] for p_ in sp["pool_op_kernel_sizes"]]
    else:                                                                      # nnUNetTrainer.py:489-501: old plans
        per_axis = [int(v) for v in sp["num_pool_per_axis"]]
        pool = [[2 if max(per_axis) - j <= i else 1 for j in per_axis] for i in range(max(per_axis))]
    if any(len(p_) != 2 or tuple(p_) not in ((2, 2), (2, 1), (1, 2)) for p_ in pool):
        _refuse("plans_per_stage[%r]['pool_op_kernel_sizes']" % stage, pool, "(2, 2), (2, 1), (1, 2)")
    conv = sp.get("conv_kernel_sizes")
    conv = [[int(v) for v in k] for k in ([[3, 3]] * (len(pool) + 1) if conv is None else conv)]
    if any(k != [3, 3] for k in conv):
        _refuse("plans_per_stage[%r]['conv_kernel_sizes']" % stage, conv, "3x3 everywhere")
    conv_per_stage = plans.get("conv_per_stage", 2)
    if conv_per_stage != 2:
        _refuse("conv_per_stage", conv_per_stage, "2")
    dp = plans.get("dataset_properties") or {}
    tf, tb = plans.get("transpose_forward"), plans.get("transpose_backward")
    if tf is None or tb is None:                                               # nnUNetTrainer.py:526-531
        tf, tb = [0, 1, 2], [0, 1, 2]
    return _plain({
        "num_modalities": int(plans["num_modalities"]),
        "num_classes": int(plans["num_classes"]) + 1,                            # nnUNetTrainer.py:520: background is not in num_classes
        "patch_size": patch,
        "mirror_axes": [0, 1],
        "seg_net": {"base_num_features": int(plans["base_num_features"]), "num_pool": len(pool), "pool_op_kernel_sizes": pool},
        "transpose_forward": [int(v) for v in tf], "transpose_backward": [int(v) for v in tb],
        "normalization_schemes": plans.get("normalization_schemes"),
        "use_mask_for_norm": plans.get("use_mask_for_norm"),
        "dataset_properties": {"intensityproperties": dp.get("intensityproperties")},
        "preprocessor_name": plans.get("preprocessor_name"),
        "plans_per_stage": stages,
        "stage": stage,
    })


def plans_from_reference_3d(plans, stage=None):
    """The reference's 3-D nnU-Net plans (experiment_planner_baseline_3DUNet.py:225-252, :343-357) -> the plans dict CineTrainer reads for a
    `3d_fullres` folder: a 3-entry patch_size, mirror_axes [0, 1, 2] and seg_net {dim: 3, base_num_features, num_pool, pool_op_kernel_sizes,
    conv_kernel_sizes} -- the Generic_UNet with conv_op = nn.Conv3d that nnUNetTrainerV2.py:147-169 builds (num_classes + 1 outputs,
    conv_per_stage 2, at most 320 filters).  The preprocessing entries are those of the 2-D translation; preprocessor_name stays as the
    plans give it (GenericPreprocessor).  A stage that holds num_blocks_encoder is the residual planner's and is translated by
    _plans_from_reference_resenc instead.

    stage=None: the only stage (nnUNetTrainer.py:478-482); with several stages, the last one -- the full-resolution stage of the
    planner's cascade order, which is the stage run_training.py hands a full-resolution trainer."""
    stages = plans["plans_per_stage"]
    if stage is None:
        stage = list(stages.keys())[0] if len(stages) == 1 else sorted(stages.keys())[-1]
    if stage not in stages:
        raise KeyError("plans_from_reference_3d: stage %r is not in plans_per_stage %s" % (stage, sorted(stages)))
    sp = stages[stage]
    patch = [int(v) for v in np.asarray(sp["patch_size"]).ravel()]
    if len(patch) != 3:
        _refuse("plans_per_stage[%r]['patch_size']" % stage, patch, "3-D stages (plans_from_reference translates 2-D ones)")
    if "num_blocks_encoder" in sp:
        return _plans_from_reference_resenc(plans, stages, stage, patch)
    if "pool_op_kernel_sizes" in sp:
        pool = [[int(v) for v in p_] for p_ in sp["pool_op_kernel_sizes"]]
    else:                                                                      # nnUNetTrainer.py:489-501: old plans
        per_axis = [int(v) for v in sp["num_pool_per_axis"]]
        pool = [[2 if max(per_axis) - j <= i else 1 for j in per_axis] for i in range(max(per_axis))]
    if any(len(p_) != 3 or any(v not in (1, 2) for v in p_) for p_ in pool):
        _refuse("plans_per_stage[%r]['pool_op_kernel_sizes']" % stage, pool, "entries of {1, 2}^3")
    if any(p_[1] != p_[2] for p_ in pool):
        _refuse("plans_per_stage[%r]['pool_op_kernel_sizes']" % stage, pool, "equal in-plane pooling")
    conv = sp.get("conv_kernel_sizes")
    conv = [[int(v) for v in k] for k in ([[3, 3, 3]] * (len(pool) + 1) if conv is None else conv)]
    if len(conv) != len(pool) + 1 or any(k not in ([1, 3, 3], [3, 3, 3]) for k in conv):
        _refuse("plans_per_stage[%r]['conv_kernel_sizes']" % stage, conv, "(1, 3, 3) or (3, 3, 3), one per stage")
    conv_per_stage = plans.get("conv_per_stage", 2)
    if conv_per_stage != 2:
        _refuse("conv_per_stage", conv_per_stage, "2")
    dp = plans.get("dataset_properties") or {}
    tf, tb = plans.get("transpose_forward"), plans.get("transpose_backward")
    if tf is None or tb is None:                                               # nnUNetTrainer.py:526-531
        tf, tb = [0, 1, 2], [0, 1, 2]
    return _plain({
        "num_modalities": int(plans["num_modalities"]),
        "num_classes": int(plans["num_classes"]) + 1,                            # nnUNetTrainer.py:520: background is not in num_classes
        "patch_size": patch,
        "mirror_axes": [0, 1, 2],
        "seg_net": {"dim": 3, "base_num_features": int(plans["base_num_features"]), "num_pool": len(pool), "pool_op_kernel_sizes": pool,
                    "conv_kernel_sizes": conv},
        "transpose_forward": [int(v) for v in tf], "transpose_backward": [int(v) for v in tb],
        "normalization_schemes": plans.get("normalization_schemes"),
        "use_mask_for_norm": plans.get("use_mask_for_norm"),
        "dataset_properties": {"intensityproperties": dp.get("intensityproperties")},
        "preprocessor_name": plans.get("preprocessor_name"),
        "plans_per_stage": stages,
        "stage": stage,
    })


def _plans_from_reference_resenc(plans, stages, stage, patch):
    """plans_from_reference_3d for a stage of the residual planner (experiment_planner_residual_3DUNet_v21.py:57-120): pool_op_kernel_sizes
    starts with the first stage's stride [1, 1, 1] and has one entry per conv_kernel_sizes entry; num_blocks_encoder / num_blocks_decoder
    give the residual blocks per encoder stage and the plain convolutions per decoder stage.  seg_net gets arch = 'resenc' -- the FabiansUNet
    nnUNetTrainerV2_ResencUNet.py:25-45 builds (num_classes + 1 outputs, features doubling up to 320)."""
    sp = stages[stage]
    where = "plans_per_stage[%r]" % stage
    pool = [[int(v) for v in p_] for p_ in sp["pool_op_kernel_sizes"]]
    if any(len(p_) != 3 or any(v not in (1, 2) for v in p_) for p_ in pool):
        _refuse("%s['pool_op_kernel_sizes']" % where, pool, "entries of {1, 2}^3")
    if any(p_[1] != p_[2] for p_ in pool):
        _refuse("%s['pool_op_kernel_sizes']" % where, pool, "equal in-plane pooling")
    if not pool or pool[0] != [1, 1, 1]:
        _refuse("%s['pool_op_kernel_sizes']" % where, pool, "a leading [1, 1, 1] (the residual planner's first-stage stride)")
    if any(p_[0] == 2 and p_[1] == 1 for p_ in pool):
        _refuse("%s['pool_op_kernel_sizes']" % where, pool, "(1, 2, 2) or (2, 2, 2) after the first entry (transposed kernels (1|2, 2, 2))")
    if any(p_ == [1, 1, 1] for p_ in pool[1:]):
        _refuse("%s['pool_op_kernel_sizes']" % where, pool, "(1, 2, 2) or (2, 2, 2) after the first entry")
    conv = [[int(v) for v in k] for k in sp["conv_kernel_sizes"]]
    if len(conv) != len(pool) or any(k not in ([1, 3, 3], [3, 3, 3]) for k in conv):
        _refuse("%s['conv_kernel_sizes']" % where, conv, "(1, 3, 3) or (3, 3, 3), one per pool_op_kernel_sizes entry")
    nenc = [int(v) for v in sp["num_blocks_encoder"]]
    if "num_blocks_decoder" not in sp:                                          # nnUNetTrainerV2_ResencUNet.py:36 reads it unconditionally
        _refuse("%s['num_blocks_decoder']" % where, None, "one positive count per stage but the bottleneck")
    ndec = [int(v) for v in sp["num_blocks_decoder"]]
    if len(nenc) != len(conv) or any(v < 1 for v in nenc):
        _refuse("%s['num_blocks_encoder']" % where, nenc, "one positive count per stage")
    if len(ndec) != len(conv) - 1 or any(v < 1 for v in ndec):
        _refuse("%s['num_blocks_decoder']" % where, ndec, "one positive count per stage but the bottleneck")
    dp = plans.get("dataset_properties") or {}
    tf, tb = plans.get("transpose_forward"), plans.get("transpose_backward")
    if tf is None or tb is None:                                               # nnUNetTrainer.py:526-531
        tf, tb = [0, 1, 2], [0, 1, 2]
    return _plain({
        "num_modalities": int(plans["num_modalities"]),
        "num_classes": int(plans["num_classes"]) + 1,                            # nnUNetTrainer.py:520: background is not in num_classes
        "patch_size": patch,
        "mirror_axes": [0, 1, 2],
        "seg_net": {"dim": 3, "arch": "resenc", "base_num_features": int(plans["base_num_features"]), "num_pool": len(pool) - 1,
                    "pool_op_kernel_sizes": pool, "conv_kernel_sizes": conv, "num_blocks_encoder": nenc, "num_blocks_decoder": ndec},
        "transpose_forward": [int(v) for v in tf], "transpose_backward": [int(v) for v in tb],
        "normalization_schemes": plans.get("normalization_schemes"),
        "use_mask_for_norm": plans.get("use_mask_for_norm"),
        "dataset_properties": {"intensityproperties": dp.get("intensityproperties")},
        "preprocessor_name": plans.get("preprocessor_name"),
        "plans_per_stage": stages,
        "stage": stage,
    })


def _stage_is_3d(plans, stage):
    """does the stage a trainer would take (stage, else the only / the last one) have a 3-entry patch?"""
    stages = plans["plans_per_stage"]
    if stage is None or stage not in stages:
        stage = sorted(stages.keys())[-1]
    return len(np.asarray(stages[stage]["patch_size"]).ravel()) == 3


def crop_and_image_size(task, successive=False):
    """(crop_size, image_size, window_size) of the flow trainers from the task folder name, substring rule for substring rule:
    SegFlowGaussian.py:117-135 (31 / 35 -> 128, 224, 7; 39 -> 192, 224, 7; else 192, 384, 8) and nnMTLTrainerV2FlowSuccessive.py:117-126
    for the successive family (which has no task-39 branch)."""
    if any(x in task for x in ("31", "35")):
        return 128, 224, 7
    if "39" in task and not successive:
        return 192, 224, 7
    return 192, 384, 8


# ------------------------------------------------------------------------------------------------ folders
def _checkpoint_folds(folder, checkpoint_name):
    """{fold number: fold directory} of the fold_<n> sub-folders that hold <checkpoint_name>.model"""
    out = {}
    for d in sorted(os.listdir(folder)):
        m = re.fullmatch(r"fold_(\d+)", d)
        if m and os.path.isfile(join(folder, d, checkpoint_name + ".model")):
            out[int(m.group(1))] = join(folder, d)
    return out


def _has_fold_dirs(folder):
    return os.path.isdir(folder) and any(re.fullmatch(r"fold_\d+", d) for d in os.listdir(folder))


def resolve_flow_folder(flow_weight_folder):
    """The `-w` folder of run_training.py (config.yaml + one <task>/fold_X/ tree) or that <task> folder itself -> (config path, task dir)."""
    w = os.path.abspath(flow_weight_folder)
    if os.path.isfile(join(w, "config.yaml")) and not _has_fold_dirs(w):
        tasks = [d for d in sorted(os.listdir(w)) if _has_fold_dirs(join(w, d))]
        if len(tasks) != 1:
            raise ValueError("%s holds config.yaml and %d task folders with fold_X/ inside (%s); pass the task folder itself"
                             % (w, len(tasks), ", ".join(tasks) or "none"))
        return join(w, "config.yaml"), join(w, tasks[0])
    if _has_fold_dirs(w) and os.path.isfile(join(os.path.dirname(w), "config.yaml")):
        return join(os.path.dirname(w), "config.yaml"), w
    raise FileNotFoundError("%s is neither a flow weight folder (config.yaml + <task>/fold_X/) nor a <task> folder under one" % w)


def _first(names, n=5):
    names = sorted(names)
    return ", ".join(names[:n]) + (" ... (%d in all)" % len(names) if len(names) > n else "")


def check_state_dict(sd, shapes, what):
    """Every tensor the network needs, no surplus, every shape equal; derived buffers (`*.grid`, `num_batches_tracked`, Swin
    `relative_position_index` / `attn_mask`) are ignored on both sides.  Missing -> KeyError, surplus or mis-shaped -> ValueError."""
    need = {k: tuple(v) for k, v in shapes.items() if not k.endswith(_DERIVED_BUFFERS)}
    have = {k: tuple(v.shape) for k, v in sd.items() if not k.endswith(_DERIVED_BUFFERS)}
    missing = set(need) - set(have)
    if missing:
        raise KeyError("%s: checkpoint lacks %d tensors the network needs: %s" % (what, len(missing), _first(missing)))
    surplus = set(have) - set(need)
    if surplus:
        raise ValueError("%s: checkpoint holds %d tensors the network does not have: %s" % (what, len(surplus), _first(surplus)))
    bad = ["%s %s (network %s)" % (k, have[k], need[k]) for k in need if have[k] != need[k]]
    if bad:
        raise ValueError("%s: %d tensors have another shape: %s" % (what, len(bad), _first(bad)))


def _trainer_info(fold_dir, checkpoint_name):
    p = join(fold_dir, checkpoint_name + ".model.pkl")
    return load_reference_pickle(p) if os.path.isfile(p) else None


def import_reference_model_folder(seg_folder, flow_weight_folder, out_folder, crop_weights=None, crop_config=None, folds=None,
                                  checkpoint_name="model_final_checkpoint", crop_size=None, image_size=None, window_size=None, seg_config=None,
                                  seg_variant=None, seg_regions=None, seg_regions_class_order=None):
    """seg_folder: output folder of a 2-D nnU-Net trainer (plans.pkl, fold_X/); flow_weight_folder: the `-w` folder of run_training.py
    (config.yaml, <task>/fold_X/) or its <task> folder; crop_weights / crop_config: optionally the MTLmodel cropper's checkpoint and its
    YAML (nnMTLTrainerV2FlowSuccessive.py:482-484, adversarial_acdc.yaml).  Writes `out_folder` in the plans.json format (save_model_folder):
    plans.json, config.yaml (+ cropping_config.yaml), one fold_X per fold, postprocessing.json when the seg folder has one.

    folds: None takes every fold, and the two folders must hold the same ones; a list selects folds that both must hold.  crop_size /
    image_size / window_size override the task-number rule (crop_and_image_size) applied to the flow trainer's dataset directory
    (`.model.pkl` init[3]; the task folder's name when that file is absent).  The flow trainer predicts on [image_size, image_size]
    patches (SegFlowGaussian.py:366), which become plans['patch_size']; the segmentation stage's own patch stays in plans_per_stage.
    flow_weight_folder=None imports the segmentation folder on its own (a segmentation-only model folder: the stage's patch size stays
    plans['patch_size'], no 'flow_net' / 'crop_size'; a cropper or crop_size / image_size / window_size make no sense then and are refused).
    A folder of a region trainer (REGION_TRAINERS, or seg_regions / seg_regions_class_order for a subclass of one's own: seg_regions_spec)
    gets seg_net.regions / seg_net.regions_class_order and num_classes = len(regions); it is segmentation-only, 2-D or 3-D Generic_UNet
    or the residual-encoder U-Net.
    Returns the plans written."""
    from . import config as C
    if not os.path.isfile(join(seg_folder, "plans.pkl")):
        raise FileNotFoundError("%s has no plans.pkl (not the output folder of an nnU-Net trainer)" % seg_folder)
    first = _checkpoint_folds(seg_folder, checkpoint_name)
    info = _trainer_info(first[sorted(first)[0]], checkpoint_name) if first else None
    if _MTL_TRAINER in str((info or {}).get("name") or ""):
        if seg_variant is not None:
            raise ValueError("seg_variant %r names a Generic_UNet trainer variant; %s was written by %s" % (seg_variant, seg_folder, info["name"]))
        if seg_regions is not None or seg_regions_class_order is not None:
            raise ValueError("seg_regions / seg_regions_class_order next to a folder of %s: seg_net.regions and seg_net.arch == 'mtl' do not go "
                             "together (MTLmodel has no region-based trainer)" % info["name"])
        if flow_weight_folder is not None:
            raise ValueError("%s was written by %s (an MTLmodel segmenter) and cannot be paired with a flow folder (-w %s): MTLmodel next to "
                             "the flow network is not built.  Import it on its own (no -w)." % (seg_folder, info["name"], flow_weight_folder))
        return _import_mtl_folder(seg_folder, out_folder, seg_config, crop_weights, crop_config, folds, checkpoint_name, crop_size, image_size,
                                  window_size)
    if seg_config is not None:
        raise ValueError("seg_config is the YAML of an %s folder; %s was written by %r" % (_MTL_TRAINER, seg_folder, (info or {}).get("name")))
    if flow_weight_folder is None:
        return _import_segmentation_only(seg_folder, out_folder, crop_weights, crop_config, folds, checkpoint_name, crop_size, image_size,
                                         window_size, seg_variant, seg_regions, seg_regions_class_order)
    if seg_regions_spec((info or {}).get("name"), seg_regions, seg_regions_class_order)[0] is not None:
        raise ValueError("%s is a region-based folder (trainer %r, seg_regions %r: seg_net.regions) and cannot be paired with a flow folder "
                         "(-w %s, flow_net): label propagation one-hot encodes exclusive labels.  Import it on its own (no -w)."
                         % (seg_folder, (info or {}).get("name"), seg_regions, flow_weight_folder))
    if _stage_is_3d(load_reference_pickle(join(seg_folder, "plans.pkl")), info["init"][5] if info and len(info.get("init") or ()) > 5 else None):
        raise ValueError("%s is a 3-D segmentation folder (3-entry patch_size) and cannot be paired with a flow folder (-w %s): the flow path "
                         "is 2-D.  Import it on its own (no -w)." % (seg_folder, flow_weight_folder))
    config_path, task_dir = resolve_flow_folder(flow_weight_folder)
    seg_folds, flow_folds = _checkpoint_folds(seg_folder, checkpoint_name), _checkpoint_folds(task_dir, checkpoint_name)
    if folds is None or folds == "None":
        if set(seg_folds) != set(flow_folds) or not seg_folds:
            raise ValueError("the two trained folders hold different folds of %s.model: segmentation %s, flow %s (pass folds=)"
                             % (checkpoint_name, sorted(seg_folds), sorted(flow_folds)))
        folds = sorted(seg_folds)
    folds = [int(f) for f in ([folds] if isinstance(folds, (int, str)) else folds)]
    for f in folds:
        for name, have, where in (("segmentation", seg_folds, seg_folder), ("flow", flow_folds, task_dir)):
            if f not in have:
                raise FileNotFoundError("fold_%d/%s.model is missing from the %s folder %s" % (f, checkpoint_name, name, where))

    seg_info = _trainer_info(seg_folds[folds[0]], checkpoint_name)
    flow_info = _trainer_info(flow_folds[folds[0]], checkpoint_name)
    stage = seg_info["init"][5] if seg_info and len(seg_info.get("init") or ()) > 5 else None
    plans = plans_from_reference(load_reference_pickle(join(seg_folder, "plans.pkl")), stage)
    row = seg_variant_row((seg_info or {}).get("name"), seg_variant)
    if row:                     # CineTrainer refuses the keys next to flow_net: a trainer variant's folder is imported on its own
        _apply_seg_variant(plans, row)
    flow_cfg = C.with_defaults(C.read_config_video(config_path), prediction=False)
    successive = "no_error" in flow_cfg and "d_model" not in flow_cfg          # config.build_flow_net's dispatch
    task = os.path.basename(str(flow_info["init"][3]).rstrip("/\\")) if flow_info and len(flow_info.get("init") or ()) > 3 else os.path.basename(task_dir)
    cs, im, win = crop_and_image_size(task, successive)
    cs, im, win = crop_size or cs, image_size or im, window_size or win
    plans.update(crop_size=int(cs), image_size=int(im), patch_size=[int(im), int(im)])
    if (crop_weights is None) != (crop_config is None):
        raise ValueError("crop_weights and crop_config go together (the MTLmodel cropper's checkpoint and its YAML)")
    crop_sd = None
    if crop_config is not None:
        plans["cropping_net"] = {"type": "mtl", "config": C.read_config(crop_config, False, False), "window_size": int(win)}
    plans["flow_net"] = {"config": flow_cfg}
    trainer = CineTrainer(plans, torch.device("cpu"))                           # builds the three networks' key / shape lists, no device work

    # every tensor of every fold is checked before anything is written
    if crop_weights is not None:
        shapes = trainer.crop_net.state_shapes()
        crop_sd = load_reference_checkpoint(crop_weights, shapes)["state_dict"]
        check_state_dict(crop_sd, shapes, "cropping network %s" % crop_weights)
        crop_sd = {k: v for k, v in crop_sd.items() if not k.endswith(_DERIVED_BUFFERS)}
    params = {}
    for f in folds:
        parts = []
        for net, fold_dir, what in ((trainer.seg_net, seg_folds[f], "segmentation"), (trainer.flow_net, flow_folds[f], "flow")):
            path = join(fold_dir, checkpoint_name + ".model")
            shapes = net.state_shapes()
            sd = load_reference_checkpoint(path, shapes)["state_dict"]
            check_state_dict(sd, shapes, "%s network %s" % (what, path))
            parts.append({k: v for k, v in sd.items() if not k.endswith(_DERIVED_BUFFERS)})
        params[f] = parts

    os.makedirs(out_folder, exist_ok=True)
    shutil.copy(config_path, join(out_folder, "config.yaml"))
    plans["flow_net"] = {"config": "config.yaml"}
    if crop_config is not None:
        shutil.copy(crop_config, join(out_folder, "cropping_config.yaml"))
        plans["cropping_net"]["config"] = "cropping_config.yaml"
    for f in folds:
        save_model_folder(out_folder, trainer.seg_net, trainer.flow_net, plans, fold=f, checkpoint_name=checkpoint_name,
                          seg_sd=params[f][0], flow_sd=params[f][1], crop_sd=crop_sd)
    if os.path.isfile(join(seg_folder, "postprocessing.json")):
        shutil.copy(join(seg_folder, "postprocessing.json"), join(out_folder, "postprocessing.json"))
    return plans


_FIRST_CONV = "conv_blocks_context.0.blocks.0.conv.weight"


def _is_cascade_stage(trainer_info, checkpoint_path, plans):
    """Is the 3-D folder the full-resolution stage of a cascade?  Either the trainer's `.model.pkl` name says so (nnUNetTrainerV2CascadeFullRes
    and its variants) or the first convolution takes num_modalities + (num_classes - 1) input channels -- `plans` is the translated dict,
    whose num_classes counts the background.  Any other width is left to check_state_dict's shape report."""
    if trainer_info and "Cascade" in str(trainer_info.get("name") or ""):
        return True
    sd = load_reference_checkpoint(checkpoint_path)["state_dict"]
    w = sd.get(_FIRST_CONV)
    return w is not None and w.dim() == 5 and int(w.shape[1]) == plans["num_modalities"] + plans["num_classes"] - 1


_ALIAS = re.compile(r"^(?P<head>.*\.convs\.\d+)\.all\.(?P<slot>\d+)\.(?P<leaf>[^.]+)$")
_ALIAS_SLOT = {"0": "conv", "2": "norm"}                                       # ConvDropoutNormReLU.all = Sequential(conv, do, norm, nonlin)


def _drop_resenc_aliases(sd, path):
    """The reference's ConvDropoutNormReLU (custom_modules/conv_blocks.py:35-52) registers its convolution and its norm twice: as `conv` /
    `norm` and as slots 0 / 2 of the nn.Sequential `all`, so a FabiansUNet checkpoint holds every decoder tensor under two names.  Each
    pair must be present and bit-equal (ValueError naming the key otherwise); the `all.*` names are dropped.  A checkpoint with BatchNorm
    running statistics is a norm_type='bn' network, which the build does not implement."""
    bn = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    if bn:
        raise NotImplementedError("%s holds BatchNorm running statistics (%s): a network built with norm_type='bn'; the build implements "
                                  "norm_type='in'" % (path, _first(bn)))
    out = {}
    for k, v in sd.items():
        m = _ALIAS.match(k)
        if m is None:
            out[k] = v
            continue
        if m.group("slot") not in _ALIAS_SLOT:
            raise ValueError("%s: %s is no slot of ConvDropoutNormReLU.all that holds tensors (0 = conv, 2 = norm)" % (path, k))
        twin = "%s.%s.%s" % (m.group("head"), _ALIAS_SLOT[m.group("slot")], m.group("leaf"))
        if twin not in sd:
            raise ValueError("%s: %s has no twin %s (ConvDropoutNormReLU registers both)" % (path, k, twin))
        if sd[twin].shape != v.shape or sd[twin].dtype != v.dtype or not torch.equal(sd[twin], v):
            raise ValueError("%s: %s and %s name one tensor of the reference's network but differ in the checkpoint" % (path, k, twin))
    for k in out:                                                              # ... and every `conv` / `norm` of a decoder stage has its alias
        m = re.match(r"^(.*\.convs\.\d+)\.(conv|norm)\.([^.]+)$", k)
        if m and k.startswith("decoder."):
            alias = "%s.all.%s.%s" % (m.group(1), "0" if m.group(2) == "conv" else "2", m.group(3))
            if alias not in sd:
                raise ValueError("%s: %s has no twin %s (ConvDropoutNormReLU registers both)" % (path, k, alias))
    return out


# ------------------------------------------------------------------------------------------------ trainer variants
# nnunet/training/network_training/nnUNet_variants/architectural_variants/: the class name `.model.pkl` holds -> what the trainer's
# initialize_network changes in Generic_UNet, as plans['seg_net'] keys (trainer.SEG_VARIANT_KEYS).  An empty row: nothing changes at
# inference.  Two private entries: 'base_num_features' (the trainer overwrites the plans' width after reading them) and 'all_conv_3x3'
# (it overwrites every conv_kernel_sizes entry with 3).  The ResencUNet trainers have their own route (seg_net.arch = 'resenc').
SEG_VARIANTS = {
    "nnUNetTrainerV2_ReLU": {"nonlin": "relu"},
    "nnUNetTrainerV2_GeLU": {"nonlin": "gelu"},                                # its GeLU module is torch.nn.functional.gelu: the erf form, CF_ACT_GELU
    "nnUNetTrainerV2_Mish": {"nonlin": "mish"},
    "nnUNetTrainerV2_LReLU_slope_2en1": {"nonlin": "lrelu", "nonlin_slope": 0.2},
    "nnUNetTrainerV2_GN": {"norm": "gn", "norm_groups": 8},                    # MyGroupNorm(num_groups=8) under the instnorm keys
    "nnUNetTrainerV2_BN": {"norm": "bn"},
    "nnUNetTrainerV2_NoNormalization": {"norm": "none"},
    "nnUNetTrainerV2_NoNormalization_lr1en3": {"norm": "none"},
    "nnUNetTrainerV2_ReLU_convReLUIN": {"nonlin": "relu", "block_order": "conv_nonlin_norm"},
    "nnUNetTrainerV2_lReLU_convReLUIN": {"block_order": "conv_nonlin_norm"},   # the class in nnUNetTrainerV2_lReLU_convlReLUIN.py
    "nnUNetTrainerV2_lReLU_convlReLUIN": {"block_order": "conv_nonlin_norm"},  # ... and that file's name
    "nnUNetTrainerV2_ReLU_biasInSegOutput": {"nonlin": "relu", "seg_output_bias": True},
    "nnUNetTrainerV2_lReLU_biasInSegOutput": {"seg_output_bias": True},
    "nnUNetTrainerV2_3ConvPerStage": {"conv_per_stage": 3, "base_num_features": 24},
    "nnUNetTrainerV2_3ConvPerStageSameFilters": {"conv_per_stage": 3},         # the class in nnUNetTrainerV2_3ConvPerStage_samefilters.py
    "nnUNetTrainerV2_3ConvPerStage_samefilters": {"conv_per_stage": 3},
    "nnUNetTrainerV2_allConv3x3": {"all_conv_3x3": True},
    "nnUNetTrainerV2_noDeepSupervision": {},                                   # the heads below full resolution exist and are never evaluated
    "nnUNetTrainerV2_softDeepSupervision": {},
    "nnUNetTrainerV2_ResencUNet": None, "nnUNetTrainerV2_ResencUNet_DA3": None, "nnUNetTrainerV2_ResencUNet_DA3_BN": None,
    # competitions_with_custom_Trainers: two BatchNorm softmax trainers (the first is no region trainer despite its name)
    "nnUNetTrainerV2BraTSRegions_BN": {"norm": "bn"},
    "nnUNetTrainerV2_MMS": {"norm": "bn"},
}

# Region-based training (competitions_with_custom_Trainers/BraTS2020): one sigmoid channel per region, num_classes = len(regions), labels
# painted in regions_class_order.  The two region sets are those of nnunet/evaluation/region_based_evaluation.py with the class orders the
# trainers set; a trainer's class name -> (region set, its SEG_VARIANTS-style row).
REGION_SETS = {
    "brats": ({"whole tumor": [1, 2, 3], "tumor core": [2, 3], "enhancing tumor": [3]}, [1, 2, 3]),
    "kits": ({"kidney incl tumor": [1, 2], "tumor": [2]}, [1, 2]),
}
_BR = "nnUNetTrainerV2BraTSRegions"
REGION_TRAINERS = {
    _BR: ("brats", {}), _BR + "_Dice": ("brats", {}), _BR + "_DDP": ("brats", {}),
    _BR + "_DA3": ("brats", {}), _BR + "_DA3_BD": ("brats", {}),
    _BR + "_DA3_BN": ("brats", {"norm": "bn"}), _BR + "_DA3_BN_BD": ("brats", {"norm": "bn"}),
    _BR + "_DA4_BN": ("brats", {"norm": "bn"}), _BR + "_DA4_BN_BD": ("brats", {"norm": "bn"}),
}


def seg_regions_spec(name, seg_regions=None, seg_regions_class_order=None):
    """(regions {name: [labels]}, regions_class_order) of a folder, or (None, None).  name: the trainer's class name (a REGION_TRAINERS row
    gives its set); seg_regions: --seg_regions, a REGION_SETS name or a JSON object / mapping {region: [labels]}, for a subclass of one's own
    (it replaces the trainer's set); seg_regions_class_order: --seg_regions_class_order (default: the named set's own order)."""
    regions = order = None
    if str(name or "") in REGION_TRAINERS:
        regions, order = REGION_SETS[REGION_TRAINERS[str(name)][0]]
    if seg_regions is not None:
        if isinstance(seg_regions, str) and seg_regions in REGION_SETS:
            regions, order = REGION_SETS[seg_regions]
        else:
            import json
            try:
                regions = json.loads(seg_regions) if isinstance(seg_regions, str) else dict(seg_regions)
            except (TypeError, ValueError) as e:
                raise ValueError("seg_regions %r is neither a region set (%s) nor a JSON object {region name: [labels]}: %s"
                                 % (seg_regions, ", ".join(sorted(REGION_SETS)), e))
            if not isinstance(regions, dict):
                raise ValueError("seg_regions %r is neither a region set (%s) nor a JSON object {region name: [labels]}"
                                 % (seg_regions, ", ".join(sorted(REGION_SETS))))
            order = None
    if seg_regions_class_order is not None:
        if regions is None:
            raise ValueError("seg_regions_class_order %r without regions: pass seg_regions (--seg_regions) too" % (seg_regions_class_order,))
        order = [int(c) for c in seg_regions_class_order]
    if regions is None:
        return None, None
    if order is None:
        raise ValueError("seg_regions given as a mapping needs seg_regions_class_order (--seg_regions_class_order): one label per region")
    return {str(k): [int(c) for c in v] for k, v in regions.items()}, [int(c) for c in order]


def check_region_head(sd, regions, trainer, path):
    """A region-based network has one output channel per region: the full-resolution head of the checkpoint must agree before
    check_state_dict's shape report can mislead (a softmax folder's head has num_classes + 1 channels)."""
    heads = sorted((int(m.group(1)), k) for k, m in ((k, re.fullmatch(r"seg_outputs\.(\d+)\.weight", k)) for k in sd) if m)
    key = heads[-1][1] if heads else ("decoder.segmentation_output.weight" if "decoder.segmentation_output.weight" in sd else None)
    if key is None:
        raise KeyError("%s: trainer %s: the checkpoint holds no segmentation head (seg_outputs.N.weight / decoder.segmentation_output.weight)"
                       % (path, trainer or "(unnamed)"))
    if int(sd[key].shape[0]) != len(regions):
        raise ValueError("%s: trainer %s: the segmentation head %s has %d output channels, but there are %d regions (%s): a region-based "
                         "network has one sigmoid channel per region (seg_regions / --seg_regions names another set)"
                         % (path, trainer or "(unnamed)", key, int(sd[key].shape[0]), len(regions), ", ".join(regions)))
_FRN = "nnUNetTrainerV2_FRN"


def seg_variant_row(name, forced=None):
    """The table row of a trainer's class name (forced: --seg_variant, a row chosen for a user's own subclass), or None: a name the table
    does not know or a ResencUNet trainer -- the import goes on as it did.  nnUNetTrainerV2_FRN is refused by name."""
    key = forced if forced is not None else str(name or "")
    if key == _FRN:
        raise NotImplementedError("%s: its 3-D network normalises with FRN3D (feature response normalisation with a learned threshold, "
                                  "custom_modules/feature_response_normalization.py), which the build does not implement, and its 2-D "
                                  "branch is BatchNorm2d(eps 1e-6) under an identity activation, which is not built either" % _FRN)
    if forced is not None and SEG_VARIANTS.get(forced) is None:
        raise ValueError("seg_variant %r is no row of the trainer-variant table (%s)" % (forced, ", ".join(k for k, v in SEG_VARIANTS.items() if v is not None)))
    return SEG_VARIANTS.get(key)


def _apply_seg_variant(plans, row):
    """the row's keys into plans['seg_net'] (the translated plans); the two private entries change base_num_features / conv_kernel_sizes"""
    sk = plans["seg_net"]
    for k, v in row.items():
        if k == "all_conv_3x3":
            if "conv_kernel_sizes" in sk:
                sk["conv_kernel_sizes"] = [[3] * len(ks) for ks in sk["conv_kernel_sizes"]]
        else:
            sk[k] = v


def check_seg_variant(sd, row, trainer, path):
    """The table row and the checkpoint must agree before check_state_dict's shape report can mislead: a ValueError that names the trainer
    and the first offending key.  row = {} for a stock trainer (or an unknown name): then the checkpoint must hold a stock network's norms."""
    what = "%s: trainer %s" % (path, trainer or "(unnamed)")
    norm = row.get("norm", "in")
    stats = sorted(k for k in sd if k.endswith((".running_mean", ".running_var")))
    norms = sorted(k for k in sd if ".instnorm." in k and not k.endswith(_DERIVED_BUFFERS))
    if norm == "bn":
        for k in sorted(k for k in sd if k.endswith(".instnorm.weight")):
            for leaf in ("running_mean", "running_var"):
                twin = k[:-len("weight")] + leaf
                if twin not in sd:
                    raise ValueError("%s builds BatchNorm (seg_net.norm = 'bn'), but the checkpoint lacks %s" % (what, twin))
        if not stats:
            raise ValueError("%s builds BatchNorm (seg_net.norm = 'bn'), but the checkpoint holds no running statistics (first norm tensor: %s)"
                             % (what, norms[0] if norms else "none"))
    elif stats:
        raise ValueError("%s builds seg_net.norm = %r, but the checkpoint holds BatchNorm running statistics: %s (a _BN trainer's folder? "
                         "--seg_variant nnUNetTrainerV2_BN)" % (what, norm, stats[0]))
    if norm == "none" and norms:
        raise ValueError("%s builds no normalisation (seg_net.norm = 'none'), but the checkpoint holds %s" % (what, norms[0]))
    biases = sorted(k for k in sd if re.fullmatch(r"seg_outputs\.\d+\.bias", k))
    heads = sorted(k for k in sd if re.fullmatch(r"seg_outputs\.\d+\.weight", k))
    if row.get("seg_output_bias", False):
        for k in heads:
            if k[:-len("weight")] + "bias" not in sd:
                raise ValueError("%s builds segmentation heads with a bias (seg_net.seg_output_bias), but the checkpoint lacks %s"
                                 % (what, k[:-len("weight")] + "bias"))
    elif biases:
        raise ValueError("%s builds bias-free segmentation heads, but the checkpoint holds %s" % (what, biases[0]))
    cps = row.get("conv_per_stage", 2)
    blocks = sorted({int(m.group(1)) for m in (re.match(r"conv_blocks_context\.0\.blocks\.(\d+)\.", k) for k in sd) if m})
    if blocks and len(blocks) != cps:
        raise ValueError("%s builds %d convolutions per stage (seg_net.conv_per_stage), but the checkpoint's first stage has %d: "
                         "conv_blocks_context.0.blocks.%d" % (what, cps, len(blocks), min(len(blocks), cps)))
    if "base_num_features" in row and _FIRST_CONV in sd and int(sd[_FIRST_CONV].shape[0]) != row["base_num_features"]:
        raise ValueError("%s sets base_num_features = %d, but %s has %d output channels"
                         % (what, row["base_num_features"], _FIRST_CONV, int(sd[_FIRST_CONV].shape[0])))


def _import_segmentation_only(seg_folder, out_folder, crop_weights, crop_config, folds, checkpoint_name, crop_size, image_size, window_size, seg_variant=None,
                              seg_regions=None, seg_regions_class_order=None):
    """import_reference_model_folder without a flow folder: every check of the segmentation side, nothing of the flow side"""
    given = {k: v for k, v in dict(crop_weights=crop_weights, crop_config=crop_config, crop_size=crop_size, image_size=image_size,
                                   window_size=window_size).items() if v is not None}
    if given:
        raise ValueError("%s belong to the flow trainer's heart-centred crop; a segmentation-only import takes none of them" % ", ".join(sorted(given)))
    seg_folds = _checkpoint_folds(seg_folder, checkpoint_name)
    if folds is None or folds == "None":
        if not seg_folds:
            raise ValueError("the segmentation folder %s holds no fold_X/%s.model" % (seg_folder, checkpoint_name))
        folds = sorted(seg_folds)
    folds = [int(f) for f in ([folds] if isinstance(folds, (int, str)) else folds)]
    for f in folds:
        if f not in seg_folds:
            raise FileNotFoundError("fold_%d/%s.model is missing from the segmentation folder %s" % (f, checkpoint_name, seg_folder))
    seg_info = _trainer_info(seg_folds[folds[0]], checkpoint_name)
    stage = seg_info["init"][5] if seg_info and len(seg_info.get("init") or ()) > 5 else None
    ref_plans = load_reference_pickle(join(seg_folder, "plans.pkl"))
    if _stage_is_3d(ref_plans, stage):                                          # a `3d_fullres` folder: checked against Generic_UNet3D below
        plans = plans_from_reference_3d(ref_plans, stage)
    else:
        plans = plans_from_reference(ref_plans, stage)
        plans["image_size"] = int(plans["patch_size"][0])
    resenc = plans["seg_net"].get("arch") == "resenc"
    name = str((seg_info or {}).get("name") or "")
    if seg_info is not None and name and (("ResencUNet" in name) != resenc):
        raise ValueError("%s: the trainer's name %r and the plans disagree -- the stage %s num_blocks_encoder, which makes it %s "
                         "residual-encoder folder" % (seg_folder, name, "holds" if resenc else "has no", "a" if resenc else "no"))
    if resenc and ("_BN" in name or name.endswith("BN")):
        raise NotImplementedError("%s: trainer %s builds its network with norm_type='bn' (BatchNorm); the build implements norm_type='in'"
                                  % (seg_folder, name))
    if not resenc and plans["seg_net"].get("dim") == 3 and _is_cascade_stage(seg_info, join(seg_folds[folds[0]], checkpoint_name + ".model"), plans):
        # a `3d_cascade_fullres` folder (nnUNetTrainerCascadeFullRes.py:87-88: num_input_channels += num_classes - 1, background excluded):
        # the previous stage's foreground labels come in as one-hot channels (predict.py:176, classes = range(1, num_classes))
        plans["seg_net"]["prev_stage_classes"] = list(range(1, plans["num_classes"]))
    row = None if resenc else seg_variant_row(name, seg_variant)
    if row is None and not resenc and seg_variant is None and name in REGION_TRAINERS:
        row = REGION_TRAINERS[name][1]                                          # the _BN region trainers build BatchNorm
    if resenc and seg_variant is not None:
        raise ValueError("seg_variant %r: %s is a residual-encoder folder, which has no trainer variants here" % (seg_variant, seg_folder))
    if row:
        _apply_seg_variant(plans, row)
    regions, order = seg_regions_spec(name, seg_regions, seg_regions_class_order)
    if regions is not None:                                                     # process_plans: self.num_classes = len(self.regions), no background
        plans["num_classes"] = len(regions)
        plans["seg_net"]["regions"], plans["seg_net"]["regions_class_order"] = regions, order
        first_path = join(seg_folds[folds[0]], checkpoint_name + ".model")
        check_region_head(load_reference_checkpoint(first_path)["state_dict"], regions, seg_variant or name, first_path)
    trainer = CineTrainer(plans, torch.device("cpu"))                           # the network's key / shape list, no device work
    params = {}
    for f in folds:                                                             # every tensor of every fold is checked before anything is written
        path = join(seg_folds[f], checkpoint_name + ".model")
        shapes = trainer.seg_net.state_shapes()
        sd = load_reference_checkpoint(path, shapes)["state_dict"]
        if resenc:
            sd = _drop_resenc_aliases(sd, path)
        else:
            check_seg_variant(sd, row or {}, seg_variant or name, path)
        if regions is not None:
            check_region_head(sd, regions, seg_variant or name, path)
        check_state_dict(sd, shapes, "segmentation network %s" % path)
        params[f] = {k: v for k, v in sd.items() if not k.endswith(_DERIVED_BUFFERS)}
    os.makedirs(out_folder, exist_ok=True)
    for f in folds:
        save_model_folder(out_folder, trainer.seg_net, None, plans, fold=f, checkpoint_name=checkpoint_name, seg_sd=params[f], flow_sd=None)
    if os.path.isfile(join(seg_folder, "postprocessing.json")):
        shutil.copy(join(seg_folder, "postprocessing.json"), join(out_folder, "postprocessing.json"))
    return plans


_MTL_TRAINER = "nnMTLTrainerV2"


def mtl_window_size(image_size):
    """nnMTLTrainerV2.py:121, value for value (None: the rule knows no window for that image size)"""
    return {224: 7, 288: 9, 384: 8, 192: 8}.get(int(image_size))


def mtl_crop_size(task):
    """the crop size of nnMTLTrainerV2.py:110-117 from the task folder's name (31 / 35 -> 128, else 192); the image and window sizes of
    those lines are overwritten at :120-121 and play no part"""
    return 128 if any(x in task for x in ("31", "35")) else 192


def _import_mtl_folder(seg_folder, out_folder, seg_config, crop_weights, crop_config, folds, checkpoint_name, crop_size, image_size, window_size):
    """A folder of nnMTLTrainerV2 (the trainer's name in `.model.pkl`) -> a seg_net.arch = 'mtl' folder.  seg_config: the trainer's YAML
    (seg_model.yaml; the copy nnMTLTrainerV2.py:488 writes as config.yaml into its log folder).  image_size = config['patch_size'][0];
    window_size by the rule of :121; with config['cropper'] the crop size by the task rule of :110-117, and the cropper's checkpoint and
    YAML are required (the trainer reads them from its working directory, :107, :601).  crop_size / image_size / window_size override the
    rules.  Every tensor of every fold and of the cropper is checked against the networks the new plans build before anything is written."""
    from . import config as C
    seg_folds = _checkpoint_folds(seg_folder, checkpoint_name)
    if folds is None or folds == "None":
        if not seg_folds:
            raise ValueError("the segmentation folder %s holds no fold_X/%s.model" % (seg_folder, checkpoint_name))
        folds = sorted(seg_folds)
    folds = [int(f) for f in ([folds] if isinstance(folds, (int, str)) else folds)]
    for f in folds:
        if f not in seg_folds:
            raise FileNotFoundError("fold_%d/%s.model is missing from the segmentation folder %s" % (f, checkpoint_name, seg_folder))
    info = _trainer_info(seg_folds[folds[0]], checkpoint_name)
    init = tuple(info.get("init") or ())
    if seg_config is None:
        raise ValueError("%s was written by %s: pass seg_config (--seg_config) -- the YAML the trainer was configured with, which it copies "
                         "as config.yaml into its log folder (nnMTLTrainerV2.py:488)" % (seg_folder, info["name"]))
    if len(init) > 9 and init[9]:
        raise NotImplementedError("%s: the trainer was built with binary = True, which is outside what the build implements" % seg_folder)
    cfg = C.read_config(seg_config, False, False)
    if cfg.get("unlabeled"):
        raise NotImplementedError("%s: unlabeled = true (ModelWrap(net1, net2)) is outside what the build implements" % seg_config)
    stage = init[5] if len(init) > 5 else None
    plans = plans_from_reference(load_reference_pickle(join(seg_folder, "plans.pkl")), stage)
    im = int(image_size or cfg["patch_size"][0])
    win = window_size or mtl_window_size(im)
    if win is None:
        raise ValueError("nnMTLTrainerV2.py:121 has no window_size for image_size %d (224 -> 7, 288 -> 9, 384 / 192 -> 8): pass window_size" % im)
    plans.update(image_size=im, patch_size=[im, im])
    plans["seg_net"] = {"arch": "mtl", "config": cfg, "window_size": int(win), "normalize": False}
    cropper = bool(cfg.get("cropper"))
    if cropper:
        if crop_weights is None or crop_config is None:
            raise ValueError("%s sets cropper: true: crop_weights and crop_config (--crop_weights, --crop_config) are required -- the "
                             "2-class MTLmodel's checkpoint and its YAML (adversarial_acdc.yaml), which the trainer reads from its working "
                             "directory (nnMTLTrainerV2.py:107, :601)" % seg_config)
        task = os.path.basename(str(init[3]).rstrip("/\\")) if len(init) > 3 and init[3] else ""
        plans["crop_size"] = int(crop_size or mtl_crop_size(task))
        plans["cropping_net"] = {"type": "mtl", "config": C.read_config(crop_config, False, False), "window_size": int(win)}
    elif crop_weights is not None or crop_config is not None or crop_size is not None:
        raise ValueError("%s sets cropper: false: crop_weights / crop_config / crop_size make no sense without the cropping network" % seg_config)
    trainer = CineTrainer(plans, torch.device("cpu"))                           # the networks' key / shape lists, no device work
    crop_sd = None
    if cropper:
        shapes = trainer.crop_net.state_shapes()
        crop_sd = load_reference_checkpoint(crop_weights, shapes)["state_dict"]
        check_state_dict(crop_sd, shapes, "cropping network %s" % crop_weights)
        crop_sd = {k: v for k, v in crop_sd.items() if not k.endswith(_DERIVED_BUFFERS)}
    params = {}
    for f in folds:                                                             # every tensor of every fold is checked before anything is written
        path = join(seg_folds[f], checkpoint_name + ".model")
        shapes = trainer.seg_net.state_shapes()
        sd = load_reference_checkpoint(path, shapes)["state_dict"]
        check_state_dict(sd, shapes, "segmentation network %s" % path)
        params[f] = {k: v for k, v in sd.items() if not k.endswith(_DERIVED_BUFFERS)}
    os.makedirs(out_folder, exist_ok=True)
    shutil.copy(seg_config, join(out_folder, "seg_config.yaml"))
    plans["seg_net"]["config"] = "seg_config.yaml"
    if cropper:
        shutil.copy(crop_config, join(out_folder, "cropping_config.yaml"))
        plans["cropping_net"]["config"] = "cropping_config.yaml"
    for f in folds:
        save_model_folder(out_folder, trainer.seg_net, None, plans, fold=f, checkpoint_name=checkpoint_name, seg_sd=params[f], flow_sd=None,
                          crop_sd=crop_sd)
    if os.path.isfile(join(seg_folder, "postprocessing.json")):
        shutil.copy(join(seg_folder, "postprocessing.json"), join(out_folder, "postprocessing.json"))
    return plans


def main(argv=None):
    parser = argparse.ArgumentParser(description="Write a cineflow model folder (plans.json + fold_X/<chk>.model) from the folders the "
                                                 "reference's trainers wrote; predict_from_folder / cineflow.predict -m take it unchanged.")
    parser.add_argument("-s", "--seg_folder", required=True, help="output folder of the 2-D nnU-Net trainer (plans.pkl, fold_X/)")
    parser.add_argument("-w", "--flow_weight_folder", required=False, default=None,
                        help="the -w folder of run_training.py (config.yaml, <task>/fold_X/) or its <task> folder; without it the segmentation folder "
                             "is imported on its own (a segmentation-only model folder)")
    parser.add_argument("-o", "--output_folder", required=True)
    parser.add_argument("--crop_weights", default=None, help="the MTLmodel cropper's model_final_checkpoint.model")
    parser.add_argument("--crop_config", default=None, help="the cropper's YAML (adversarial_acdc.yaml)")
    parser.add_argument("--seg_config", default=None, help="for a folder of nnMTLTrainerV2: the trainer's YAML (seg_model.yaml / the config.yaml "
                                                           "it wrote into its log folder); the folder is then imported as an MTLmodel segmenter, without -w")
    parser.add_argument("--seg_variant", default=None, metavar="NAME",
                        help="build the segmentation network as this trainer variant does (a class name of nnUNet_variants/architectural_variants, "
                             "e.g. nnUNetTrainerV2_BN), whatever name the folder's .model.pkl holds: for a subclass of one's own")
    parser.add_argument("--seg_regions", default=None, metavar="NAME_OR_JSON",
                        help="the folder is region-based (one sigmoid channel per region): 'brats' or 'kits' (the region sets of "
                             "region_based_evaluation.py) or a JSON object {region name: [labels]} in channel order; for a subclass of one's own -- "
                             "the nnUNetTrainerV2BraTSRegions* trainers are recognised by name")
    parser.add_argument("--seg_regions_class_order", nargs="+", type=int, default=None, metavar="L",
                        help="the label each region paints, in channel order (a later region overwrites an earlier one); default: the named set's own")
    parser.add_argument("-f", "--folds", nargs="+", default="None")
    parser.add_argument("-chk", default="model_final_checkpoint", required=False)
    parser.add_argument("--crop_size", type=int, default=None)
    parser.add_argument("--image_size", type=int, default=None)
    parser.add_argument("--window_size", type=int, default=None)
    a = parser.parse_args(argv)
    plans = import_reference_model_folder(a.seg_folder, a.flow_weight_folder, a.output_folder, a.crop_weights, a.crop_config,
                                          None if a.folds == "None" else a.folds, a.chk, a.crop_size, a.image_size, a.window_size, a.seg_config, a.seg_variant,
                                          a.seg_regions, a.seg_regions_class_order)
    if plans["seg_net"].get("arch") == "mtl":
        print("wrote %s (MTLmodel segmenter, image %d, crop %s, window %d, %d classes)" % (a.output_folder, plans["image_size"], plans.get("crop_size"),
                                                                                        plans["seg_net"]["window_size"], plans["num_classes"]))
    elif "flow_net" not in plans:
        print("wrote %s (segmentation only, patch %s, %d classes)" % (a.output_folder, plans["patch_size"], plans["num_classes"]))
    else:
        print("wrote %s (crop %d, image %d, %d classes)" % (a.output_folder, plans["crop_size"], plans["image_size"], plans["num_classes"]))


if __name__ == "__main__":
    main()
