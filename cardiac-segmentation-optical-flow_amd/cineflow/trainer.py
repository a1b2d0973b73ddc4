"""The trainer duck type behind cineflow.predict, and the model folder it is loaded from.

Differences from the reference that are deliberate and documented in DESIGN.md (the file-level ones are listed in cineflow.predict):
  * the model folder holds `plans.json` + `fold_X/<chk>.model` written by `save_model_folder` below (a plain tensor
    dict, loaded with `torch.load(weights_only=True)`), one folder for both networks; the folders the reference's trainers
    write (`plans.pkl`, `fold_X/<chk>.model` + `.model.pkl`, the flow trainer's `config.yaml` + `<task>/fold_X/`) are turned
    into one by `cineflow.reference_models` (restricted unpickler, tensor names and shapes checked), never read here;
  * every selected fold is used (`folds=None`: every `fold_X`): `CineTrainer.load_ensemble` keeps one packed segmentation U-Net per fold
    resident and the segmentation softmax is the mean over the folds of each fold's flip-TTA softmax (what predict.py:952-960 / :1074-1082
    intend; as written those lines cannot run with more than one fold).  The flow comes from the first selected fold's flow network only
    (in the reference only params[0] ever produces one, :318 / :1028), flow fields are never averaged, and the propagated labels are the
    arg-max of the ensembled ED softmax warped with that flow.
"""
import glob
import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ops, parallel, preprocessing
from .inference import (CroppingNet, Processor, _predict_cine_tiled_device, normalize_intensity_, pad_nd_image, predict_3D_2Dconv_tiled,
                        predict_3D_3Dconv_tiled, predict_cine_2Dconv_tiled, predict_cine_slices)
from .models import FabiansUNet3D, Generic_UNet, Generic_UNet3D, SegFlowGaussian

join = os.path.join

API_PROFILE = os.environ.get("CF_API_PROFILE", "0") != "0"
DEVICE_SPLIT = {}                                                    # CF_API_PROFILE=1: prepare / networks / finish seconds inside the device batches


# ------------------------------------------------------------------------------------------------ model folder
def save_model_folder(folder, seg_net, flow_net, plans, fold=0, checkpoint_name="model_final_checkpoint", seg_sd=None, flow_sd=None, crop_sd=None):
    """Write `<folder>/plans.json` and `<folder>/fold_<fold>/<checkpoint_name>.model` (state dicts keyed by the
    reference's parameter names).  `seg_sd` / `flow_sd` / `crop_sd` (the Processor's cropping network, plans['cropping_net']): {name: tensor}.
    A segmentation-only folder (plans without 'flow_net') is written with flow_net = flow_sd = None: the checkpoint then has no
    'flow_state_dict'."""
    os.makedirs(join(folder, "fold_%d" % fold), exist_ok=True)
    with open(join(folder, "plans.json"), "w") as f:
        json.dump(plans, f, indent=1)
    ck = {"seg_state_dict": {k: v.cpu() for k, v in seg_sd.items()}}
    if flow_sd is not None:
        ck["flow_state_dict"] = {k: v.cpu() for k, v in flow_sd.items()}
    if crop_sd is not None:
        ck["crop_state_dict"] = {k: v.cpu() for k, v in crop_sd.items()}
    torch.save(ck, join(folder, "fold_%d" % fold, checkpoint_name + ".model"))


def default_plans(image_size=256, crop_size=None, flow_variant="video", seg_base=32, seg_pool=6, reduced=None):
    """flow_variant=None: the plans of a segmentation-only model (no 'flow_net', no 'crop_size')."""
    p = {"num_modalities": 1, "num_classes": 4, "patch_size": [image_size, image_size], "transpose_forward": [0, 1, 2],
         "transpose_backward": [0, 1, 2], "mirror_axes": [0, 1], "crop_size": crop_size or image_size, "image_size": image_size,
         "seg_net": {"base_num_features": seg_base, "num_pool": seg_pool},
         "flow_net": {"variant": flow_variant, "kwargs": reduced or {}}}
    if flow_variant is None:
        del p["flow_net"], p["crop_size"]
    return p


def _config_values(spec, model_folder, reader):
    """a config given inline (the YAML's mapping) or as a file name, absolute or relative to the model folder"""
    if isinstance(spec, dict):
        return spec
    path = spec if os.path.isabs(spec) or model_folder is None else join(model_folder, spec)
    return reader(path)


class ModelWrapFlow:
    """ModelWrap (successive.yaml: Optical_flow_model_successive.py:58-134) behind the flow-network interface of predict_cine_slices:
    __call__(x [T,B,1,H,W]) -> {'backward_flow': ED->t cumulative flow [T-1,B,2,H,W]} (out2['cumulated'], or model1's single pair flow
    when T == 2, :95-96)."""
    num_classes = 4

    def __init__(self, wrap):
        self.wrap = wrap

    def __call__(self, x):
        _out1, out2 = self.wrap(x, inference=False)
        return {"backward_flow": out2["cumulated"] if x.shape[0] > 2 else out2["flow"][None]}

    def state_shapes(self):
        return self.wrap.state_shapes()

    def load_state_dict(self, sd, device, **kw):
        self.wrap.load_state_dict(sd, device, **kw)
        return self


# `mixed_precision=True` (the reference's default) is honoured only on request: measured on the seeded networks, the one-term segmentation path
# misses the 1e-3 Dice bar (per-class Dice 0.992-0.999 against the f32-class path, tests/test_gpu_models.py::test_generic_unet_mixed_precision_measured,
# bench.py --seg-precision f16), so by default the flag is accepted and every network stays f32-class.  CF_SEG_MIXED_PRECISION=1 turns it on.
SEG_MIXED_PRECISION = os.environ.get("CF_SEG_MIXED_PRECISION", "0") == "1"


class CineTrainer:
    """Duck-types the trainer interface `predict_cases` uses (predict.py:285-354, :1028-1091).

    plans['flow_net'] selects the flow network either the build's short way, {'variant': 'video' | 'raft_config', 'kwargs': {...}}, or the
    reference's way, {'config': <mapping of the YAML's values, or a file name such as 'config.yaml' in the model folder>}: that config goes
    through cineflow.config (`read_config_video` + `build_seg_flow_gaussian_model` / the successive pair), as run_training.py:191 does with
    `<weights>/config.yaml`.  `prediction: false` is supplied when the file lacks it (raft_config.yaml).
    plans['cropping_net'] = {'type': 'mtl', 'config': <adversarial_acdc.yaml values or file name>, 'window_size': 7} puts the reference's own
    cropping network -- MTLmodel(num_classes=2), voxelmorph_saver_Lib.py:340-348 -- into the Processor; {'base_num_features', 'num_pool'}
    keeps the 2-class Generic_UNet stand-in of round 2.
    Plans without 'flow_net' (or with null) describe a segmentation-only model -- a plain 2-D nnU-Net folder: `flow_net` is None, neither
    'crop_size' nor a cropping network is needed, and the file-level API takes the reference's predict_non_flow route (predict.py:320-353).
    `seg_nets` holds one packed Generic_UNet per selected fold (`load_ensemble`); `seg_net` is seg_nets[0].
    plans['seg_net']['prev_stage_classes'] (a list of label values, e.g. [1, 2, 3]) makes the model the full-resolution stage of a cascade
    (`3d_cascade_fullres`, nnUNetTrainerCascadeFullRes.py:87-88): the network takes num_modalities + len(classes) input channels, and
    preprocess_patient appends the previous stage's labels as one-hot channels.  3-D segmentation-only models alone.
    plans['seg_net']['arch'] = 'resenc' (with num_blocks_encoder / num_blocks_decoder, and a pool_op_kernel_sizes list that starts with the
    first stage's stride [1, 1, 1]) makes the network the residual-encoder U-Net of nnUNetTrainerV2_ResencUNet (FabiansUNet3D): 3-D
    segmentation-only models alone, never a cascade stage.
    plans['seg_net'] = {'arch': 'mtl', 'config': <seg_model.yaml values or file name>, 'window_size': 7, 'normalize': false} makes the network
    the fork's own MTLmodel (nnMTLTrainerV2): 2-D segmentation-only models alone, patch_size = [image_size, image_size]; built at
    crop_size behind the Processor when the plans hold a cropping_net, at image_size without one (nnMTLTrainerV2.py:598-610); every
    fold's segmenter shares the one Processor, and tile batches go through MTLmodel.accumulate_tta_batch (inference.ensemble_predict_2d).
    With 'arch' absent, plans['seg_net'] may hold the choices of nnU-Net's architectural trainer variants (SEG_VARIANT_KEYS: norm,
    norm_groups, nonlin, nonlin_slope, conv_per_stage, block_order, seg_output_bias; cascade stages included): Generic_UNet / Generic_UNet3D
    are then built as that trainer built them, in every fold of load_ensemble.  Without them the network is the stock one; next to 'arch'
    or 'flow_net', or with an unknown value, each is refused."""

    def __init__(self, plans, device, model_folder=None):
        self.plans = plans
        self.device = device
        self.num_classes = plans["num_classes"]
        self.data_aug_params = {"mirror_axes": tuple(plans["mirror_axes"])}
        self.patch_size = tuple(plans["patch_size"])
        fk = plans.get("flow_net")
        self.seg_dim = int((plans.get("seg_net") or {}).get("dim", 2))
        arch = (plans.get("seg_net") or {}).get("arch")
        self.regions, self.regions_class_order = _check_regions(plans, arch, fk)      # both None unless the folder is region-based
        if arch == "mtl":
            _check_mtl_plans(plans, self.seg_dim, fk)
        elif arch is not None:
            if arch != "resenc":
                raise ValueError("seg_net.arch must be 'resenc' (the residual-encoder U-Net), 'mtl' (MTLmodel) or absent (Generic_UNet), got %r" % (arch,))
            if self.seg_dim != 3:
                raise ValueError("plans.json holds seg_net.arch == 'resenc' with seg_net.dim == %d: the residual-encoder U-Net is built in 3-D "
                                 "only (the reference's 2-D branch cannot be built either)" % self.seg_dim)
            if fk:
                raise ValueError("plans.json holds both seg_net.arch == 'resenc' and flow_net: the flow path is 2-D (a residual-encoder folder is "
                                 "segmentation-only)")
            if (plans.get("seg_net") or {}).get("prev_stage_classes") is not None:
                raise ValueError("plans.json holds both seg_net.arch == 'resenc' and seg_net.prev_stage_classes: the reference has no cascade "
                                 "trainer for the residual-encoder U-Net")
        self.seg_variant = _seg_variant_kwargs(plans.get("seg_net") or {}, arch, fk)
        if self.seg_dim == 3:
            if fk:
                raise ValueError("plans.json holds both seg_net.dim == 3 and flow_net: the flow path is 2-D (a 3-D segmentation folder is segmentation-only)")
            if len(plans["patch_size"]) != 3:
                raise ValueError("seg_net.dim == 3 needs a 3-entry patch_size, got %r" % (plans["patch_size"],))
        psc = (plans.get("seg_net") or {}).get("prev_stage_classes")
        if psc is not None:
            if self.seg_dim != 3:
                raise ValueError("plans.json holds seg_net.prev_stage_classes with seg_net.dim == %d: only a 3-D model can be the full-resolution "
                                 "stage of a cascade (nnU-Net has no 2-D cascade)" % self.seg_dim)
            if fk:
                raise ValueError("plans.json holds both seg_net.prev_stage_classes and flow_net: a cascade stage is segmentation-only")
            if not isinstance(psc, (list, tuple)) or not psc or any(not isinstance(c, int) or isinstance(c, bool) or not 0 <= c <= 255 for c in psc):
                raise ValueError("seg_net.prev_stage_classes must be a non-empty list of label values in 0..255, got %r" % (psc,))
        self.prev_stage_classes = None if psc is None else [int(c) for c in psc]
        self.seg_arch = arch
        self.model_folder = model_folder
        # (a segmentation-only model has no heart-centred crop: no Processor)
        # (an MTLmodel segmenter crops only with a cropping network: nnMTLTrainerV2.py:598-606 builds no Processor without one)
        has_crop = (fk or "crop_size" in plans) and not (arch == "mtl" and not plans.get("cropping_net"))
        self.processor = Processor(crop_size=plans["crop_size"], image_size=plans["patch_size"][0]) if has_crop else None
        # mixed_precision of load_model_and_checkpoint_files / predict_from_folder (the reference's default True): with CF_SEG_MIXED_PRECISION=1
        # the segmentation U-Net runs its convolutions in the one-term fp16 product mode (ops.conv_terms(1)), like the reference's autocast on
        # that path (neural_network.py:140-146); the flow network never does (SegFlowGaussian.py:2905-2909).  Default: flag accepted, f32-class.
        self.mixed_precision = False
        self.crop_net = None
        ck = plans.get("cropping_net") if self.processor is not None else None
        if ck:
            if ck.get("type") == "mtl":
                from . import config as C
                cfg = _config_values(ck["config"], model_folder, lambda f: C.read_config(f, False, False))
                self.crop_net = C.build_2d_model(cfg, conv_layer=None, norm=None, log_function=None, image_size=plans["patch_size"][0],
                                                 window_size=ck["window_size"], middle=False, num_classes=2, processor=None)
                self.processor.cropping_network = self.crop_net            # MTLmodel.forward returns {'pred': logits} itself
            else:
                self.crop_net = Generic_UNet(1, ck["base_num_features"], 2, ck["num_pool"])
                self.processor.cropping_network = CroppingNet(self.crop_net)
        self.seg_net = self._new_seg_net()
        self.seg_nets = [self.seg_net]                                           # one network per selected fold (load_ensemble)
        if not fk:
            self.flow_net = None
        elif fk.get("config") is not None:
            from . import config as C
            cfg = C.with_defaults(_config_values(fk["config"], model_folder, C.read_config_video), prediction=False)
            net = C.build_flow_net(cfg, image_size=plans["crop_size"])
            self.flow_net = ModelWrapFlow(net) if not isinstance(net, SegFlowGaussian) else net
        else:
            ma = fk["variant"] == "raft_config"
            kw = dict(image_size=plans["crop_size"], motion_appearance=ma, dim_feedforward=3072 if ma else 2048)
            kw.update(fk.get("kwargs", {}))
            self.flow_net = SegFlowGaussian(**kw)

    def _new_seg_net(self):
        net = self._build_seg_net()
        if self.regions is not None:        # nnUNetTrainerV2BraTSRegions.initialize_network: self.network.inference_apply_nonlin = nn.Sigmoid()
            net.inference_apply_nonlin = "sigmoid"
        return net

    def _build_seg_net(self):
        sk = self.plans["seg_net"]
        if self.seg_arch == "mtl":      # nnMTLTrainerV2.py:608-610: MTLmodel at the crop size behind a Processor, at the image size without one
            from . import config as C
            cfg = _config_values(sk["config"], self.model_folder, lambda f: C.read_config(f, False, False))
            size = self.plans["crop_size"] if self.processor is not None else self.plans["image_size"]
            net = C.build_2d_model(cfg, conv_layer=None, norm=None, log_function=None, image_size=size, window_size=sk["window_size"],
                                   middle=False, num_classes=self.num_classes, processor=self.processor)
            net.normalize = bool(sk.get("normalize", False))
            return net
        if self.seg_arch == "resenc":   # nnUNetTrainerV2_ResencUNet: FabiansUNet with conv_op = nn.Conv3d, at most 320 filters
            return FabiansUNet3D(self.plans["num_modalities"], sk["base_num_features"], sk["num_blocks_encoder"], sk["pool_op_kernel_sizes"],
                                 sk["conv_kernel_sizes"], self.num_classes, sk["num_blocks_decoder"])
        if self.seg_dim == 3:           # a `3d_fullres` stage: Generic_UNet with conv_op = nn.Conv3d, at most MAX_NUM_FILTERS_3D = 320 filters
            return Generic_UNet3D(self.plans["num_modalities"] + len(self.prev_stage_classes or ()), sk["base_num_features"], self.num_classes, sk["num_pool"],
                                  pool_op_kernel_sizes=sk.get("pool_op_kernel_sizes"), conv_kernel_sizes=sk.get("conv_kernel_sizes"), **self.seg_variant)
        return Generic_UNet(self.plans["num_modalities"], sk["base_num_features"], self.num_classes, sk["num_pool"],
                            pool_op_kernel_sizes=sk.get("pool_op_kernel_sizes"),     # the plans' per-stage pooling (plans_per_stage[...]['pool_op_kernel_sizes'])
                            **self.seg_variant)

    # -- network_trainer.py:418 load_checkpoint_ram(params, train)
    def load_checkpoint_ram(self, params, train=False):
        """one fold: its weights go into seg_net / flow_net / crop_net, and the ensemble is that fold alone"""
        self.seg_net.load_state_dict(params["seg_state_dict"], self.device)
        self.seg_nets = [self.seg_net]
        if self.flow_net is not None:
            if "flow_state_dict" not in params:
                raise KeyError("plans['flow_net'] is set but the checkpoint has no 'flow_state_dict' (a segmentation-only checkpoint)")
            self.flow_net.load_state_dict(params["flow_state_dict"], self.device)
        if self.crop_net is not None:
            if "crop_state_dict" not in params:
                raise KeyError("plans['cropping_net'] is set but the checkpoint has no 'crop_state_dict' (save_model_folder(..., crop_sd=...))")
            self.crop_net.load_state_dict(params["crop_state_dict"], self.device)

    def load_ensemble(self, params_list):
        """Every selected fold resident at once: fold 0 loads exactly as load_checkpoint_ram loads it (segmentation, flow and cropping
        networks); every further fold gets a Generic_UNet of its own, built and packed here, once -- its f16 / Winograd weight forms are
        derived on first use and then kept, never re-packed per batch.  The flow and the cropping network are fold 0's alone: in the
        reference only params[0] ever produces a flow (predict.py:318, :1028)."""
        assert len(params_list) >= 1
        self.load_checkpoint_ram(params_list[0], False)
        nets = [self.seg_net]
        for p_ in params_list[1:]:
            net = self._new_seg_net()
            net.load_state_dict(p_["seg_state_dict"], self.device)
            nets.append(net)
        self.seg_nets = nets

    # -- nnUNetTrainer.py:571-597 preprocess_patient(list_of_files) -> (data[C,Z,Y,X], seg, properties)
    def check_prev_stage(self, given):
        """a cascade stage needs the previous stage's labels and no other model takes them (the reference ends both cases in a
        channel-count crash inside the first convolution)"""
        _check_prev_stage(self.prev_stage_classes, given, self.model_folder)

    def preprocess_patient(self, input_files, seg_from_prev_stage=None):
        """Crop to non-zero, resample to the stage's spacing and normalise on the device (cineflow.preprocessing), driven by the
        same plan entries as the reference: preprocessor_name (default PreprocessorFor2D -- the fork's networks are 2-D),
        normalization_schemes, use_mask_for_norm, transpose_forward, dataset_properties.intensityproperties and
        plans_per_stage[stage].current_spacing (absent: the case keeps its own spacing).
        seg_from_prev_stage: the previous stage's label file of this case (predict.py:68-85), for a model with seg_net.prev_stage_classes: data
        then has num_modalities + len(classes) channels."""
        self.check_prev_stage(seg_from_prev_stage is not None)
        prev = {} if seg_from_prev_stage is None else {"seg_from_prev_stage": seg_from_prev_stage, "prev_stage_classes": self.prev_stage_classes}
        plans = self.plans
        nmod = plans["num_modalities"]
        as_int_keys = lambda d, default: {int(k): v for k, v in (d or {c: default for c in range(nmod)}).items()}   # noqa: E731  (JSON keys are strings)
        schemes = as_int_keys(plans.get("normalization_schemes"), "nonCT")
        use_mask = as_int_keys(plans.get("use_mask_for_norm"), False)
        ip = (plans.get("dataset_properties") or {}).get("intensityproperties")
        ip = None if ip is None else {int(k): v for k, v in ip.items()}
        name = plans.get("preprocessor_name") or "PreprocessorFor2D"
        cls = getattr(preprocessing, name, None)
        assert cls is not None, "Could not find preprocessor %s in cineflow.preprocessing" % name
        pre = cls(schemes, use_mask, list(plans["transpose_forward"]), ip)
        stages = plans.get("plans_per_stage")
        if stages:
            st = stages[str(plans.get("stage", 0))] if isinstance(stages, dict) and str(plans.get("stage", 0)) in stages else stages[plans.get("stage", 0)]
            return pre.preprocess_test_case(list(input_files), np.array(st["current_spacing"], dtype=float), **prev)
        return pre.preprocess_test_case(list(input_files), None, **prev)      # (no stages in the plans: the case keeps its own spacing)

    # -- nnUNetTrainer.py:637-679
    def predict_preprocessed_data_return_seg_and_softmax(self, data, do_mirroring=True, mirror_axes=None, use_sliding_window=True,
                                                         step_size=0.5, use_gaussian=True, pad_border_mode="constant", pad_kwargs=None,
                                                         all_in_gpu=False, verbose=True, mixed_precision=True, return_device=False):
        """(seg [Z,X,Y], softmax [K,Z,X,Y]) of one preprocessed volume; with several folds resident (load_ensemble) the softmax is the
        mean over the folds of each fold's flip-TTA sliding-window softmax.  return_device: the same two as device tensors (views of the
        padded buffers, not necessarily contiguous), nothing copied to the host (cineflow.validate resamples and scores them there)."""
        mirror_axes = self.data_aug_params["mirror_axes"] if mirror_axes is None else mirror_axes
        with ops.conv_terms(1 if (mixed_precision and SEG_MIXED_PRECISION) else 3):
            if self.seg_dim == 3:
                seg, prob = self._predict_volume_3d(data, step_size, do_mirroring, mirror_axes, use_gaussian, pad_border_mode, pad_kwargs)
                return (seg, prob) if return_device else (seg.cpu().numpy(), prob.cpu().numpy())
            if len(self.seg_nets) == 1 and self.seg_arch != "mtl":
                return predict_3D_2Dconv_tiled(self.seg_net, data, self.patch_size, step_size=step_size, do_mirroring=do_mirroring,
                                               mirror_axes=mirror_axes, use_gaussian=use_gaussian, pad_border_mode=pad_border_mode,
                                               pad_kwargs=pad_kwargs, return_device=return_device, regions_class_order=self.regions_class_order)
            if return_device:
                return _predict_cine_tiled_device(self.seg_nets, [data], self.patch_size, step_size, do_mirroring, mirror_axes, use_gaussian,
                                                  pad_border_mode, pad_kwargs, None, self.regions_class_order)[0]
            return predict_cine_2Dconv_tiled(self.seg_nets, [data], self.patch_size, step_size=step_size, do_mirroring=do_mirroring,
                                             mirror_axes=mirror_axes, use_gaussian=use_gaussian, pad_border_mode=pad_border_mode,
                                             pad_kwargs=pad_kwargs, regions_class_order=self.regions_class_order)[0]

    def _predict_volume_3d(self, data, step_size, do_mirroring, mirror_axes, use_gaussian, pad_border_mode, pad_kwargs):
        """One volume [C,Z,Y,X] through predict_3D_3Dconv_tiled, one fold at a time, everything on the device: (seg uint8, softmax).  Several
        folds: the softmax is the fold mean -- each fold's sliding-window softmax added in fold order, each with weight 1 / folds as in the
        2-D ensemble -- and the labels are its arg-max; one fold: predict_3D_3Dconv_tiled's own labels.  A region-based folder: the
        labels are the region rule (regions_class_order) on the same probabilities, one fold or the fold mean."""
        acc = seg = None
        n = len(self.seg_nets)
        for net in self.seg_nets:
            seg, prob = predict_3D_3Dconv_tiled(net, data, self.patch_size, step_size, do_mirroring, mirror_axes, use_gaussian, pad_border_mode,
                                                pad_kwargs, return_device=True, regions_class_order=self.regions_class_order)
            if n == 1:
                return seg, prob
            prob = prob.contiguous().mul_(1.0 / n)
            acc = prob if acc is None else ops.add(acc, prob, out=acc)
        K, Z, Y, X = acc.shape
        if self.regions_class_order is not None:
            return ops.region_labels(acc[None], self.regions_class_order)[0], acc
        return ops.argmax_channels(acc.view(1, K, Z * Y, X)).view(Z, Y, X), acc

    def predict_volumes_seg(self, volumes, do_mirroring=True, mirror_axes=None, step_size=0.5, use_gaussian=True, pad_border_mode="constant",
                            pad_kwargs=None, mixed_precision=True, want_softmax=True):
        """The segmentation-only device stage of the file-level API: every volume [C,Z,Y,X] of a patient group (all frames of all its
        patients) through predict_cine_2Dconv_tiled's device path in ONE call, all resident folds ensembled.  Returns per volume
        (seg uint8 [Z,Y,X], softmax [K,Z,Y,X] or None) as host arrays (pinned staging, one synchronisation)."""
        mirror_axes = self.data_aug_params["mirror_axes"] if mirror_axes is None else mirror_axes
        with ops.conv_terms(1 if (mixed_precision and SEG_MIXED_PRECISION) else 3):
            if self.seg_dim == 3:
                res = [self._predict_volume_3d(v, step_size, do_mirroring, mirror_axes, use_gaussian, pad_border_mode, pad_kwargs) for v in volumes]
            else:
                res = _predict_cine_tiled_device(self.seg_nets, volumes, self.patch_size, step_size, do_mirroring, mirror_axes, use_gaussian,
                                                 pad_border_mode, pad_kwargs, None, self.regions_class_order)
        dev_out = []
        for s_, p_ in res:
            dev_out.append(s_.contiguous())
            if want_softmax:
                dev_out.append(p_.contiguous())
        host = self._to_host(dev_out)
        if want_softmax:
            return [(host[2 * i], host[2 * i + 1]) for i in range(len(res))]
        return [(h, None) for h in host]

    # -- SegFlowGaussian.py:3294-3533 up to the network call: pad, centre crop to the patch, heart-centred crop, z-score
    def _flow_prepare(self, unlabeled, target, processor, pad_border_mode, pad_kwargs, centroid):
        T, _, Z, Y, X = unlabeled.shape
        P = self.patch_size
        x = unlabeled[:, 0]                                                            # [T,Z,Y,X]
        data, slicer = pad_nd_image(x, P, pad_border_mode, pad_kwargs, True)            # SegFlowGaussian.py:3310
        Hp, Wp = data.shape[-2:]
        y1, y2 = int(Hp / 2 - P[0] / 2), int(Hp / 2 + P[0] / 2)                         # :3391-3397 centre crop to the patch
        x1, x2 = int(Wp / 2 - P[1] / 2), int(Wp / 2 + P[1] / 2)
        dev = self.device
        patch = torch.from_numpy(np.ascontiguousarray(data[:, :, y1:y2, x1:x2])).to(dev, dtype=torch.float32)   # [T,Z,P,P]
        cs = processor.crop_size
        # one cropping window per slice (SegFlowGaussian.py:3099-3103 runs per slice): around the caller's centroid, else around the mean
        # centroid of the cropping network's masks (processor.py:232-237), else around the patch centre
        wins = []
        for z in range(Z):
            if centroid is not None:
                cen = centroid
            elif getattr(processor, "cropping_network", None) is not None:
                cen = [int(v) for v in processor.preprocess_no_registration(patch[:, z].unsqueeze(1).contiguous())[0]]
            else:
                cen = (P[1] // 2, P[0] // 2)
            wins.append(processor.adjust_cropping_window(cen))
        crop = torch.empty((T, Z, cs, cs), dtype=torch.float32, device=dev)
        for z in range(Z):
            cx0, cx1, cy0, cy1 = wins[z]["crop_indices"]
            blk = ops.crop2d(patch[:, z].contiguous(), cy0, cx0, cs, cs)               # [T,cs,cs]
            normalize_intensity_(blk)                                                   # :3108 NormalizeIntensity on the slice's [T,h,w] block
            crop[:, z] = blk
        ed = None
        if target is not None:
            tp = pad_nd_image(np.asarray(target)[None], P, "constant", {"constant_values": 0}, False)[0]
            tp = tp[:, y1:y2, x1:x2]
            ed = torch.from_numpy(np.ascontiguousarray(np.stack([tp[z, wins[z]["crop_indices"][2]:wins[z]["crop_indices"][3],
                                                                    wins[z]["crop_indices"][0]:wins[z]["crop_indices"][1]] for z in range(Z)]))).to(dev, dtype=torch.uint8)
        pad_need = np.stack([np.asarray(w["padding_need"], dtype=np.int64) for w in wins], axis=1)     # [4, Z]
        return {"frames": crop.view(T, Z, 1, cs, cs), "ed": ed, "pad_need": pad_need, "slicer": slicer, "geom": (T, Z, Y, X, Hp, Wp, y1, y2, x1, x2),
                "processor": processor}

    @staticmethod
    def _to_host(tensors):
        """device tensors -> numpy arrays through pinned staging buffers (torch's caching host allocator), one synchronisation for all of
        them: the per-patient results are ~0.5 GB, pageable `.cpu()` copies were a fifth of the API's device stage"""
        hosts = []
        for t in tensors:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            hosts.append(h)
        torch.cuda.current_stream().synchronize()
        return [h.numpy() for h in hosts]

    # -- :3427-3467 after the network call: per-slice uncrop, centre window, un-pad, host copies
    def _flow_finish(self, prep, out, return_crop, want_raw=True, want_softmax=True):
        T, Z, Y, X, Hp, Wp, y1, y2, x1, x2 = prep["geom"]
        processor, pad_need, slicer, frames, dev = prep["processor"], prep["pad_need"], prep["slicer"], prep["frames"], self.device

        def place(t):  # [T, C?, Z, cs, cs] -> [..., Z, Y, X]: per-slice uncrop (processor.py:178-186), centre window, un-pad
            zax = t.dim() - 3
            full = torch.stack([processor.uncrop_no_registration(t.select(zax, z).contiguous(), pad_need[:, z]) for z in range(Z)], dim=zax)
            canvas = torch.zeros(tuple(full.shape[:-2]) + (Hp, Wp), dtype=full.dtype, device=dev)
            canvas[..., y1:y2, x1:x2] = full
            return canvas[..., slicer[-2], slicer[-1]]

        softmax = place(out["softmax"].permute(0, 2, 1, 3, 4).contiguous())            # [T,K,Z,Y,X]
        flow = place(out["flow"].permute(0, 2, 1, 3, 4).contiguous())                  # [T,2,Z,Y,X]
        reg = place(out["registered"].float())[:, None]                                # [T,1,Z,Y,X]
        seg = ops.argmax_channels(softmax.reshape(T, self.num_classes, -1).contiguous()).view(T, Z, Y, X)
        # (want_softmax=False: the exporter will write the device arg-max `seg`; the [T,K,Z,Y,X] probabilities -- 200 MB per patient -- stay on the device)
        dev_out = [seg, softmax.contiguous() if want_softmax else torch.empty(0, device=dev), flow.contiguous(), reg.contiguous()]
        if want_raw:
            dev_out.append(torch.cat([frames.permute(0, 2, 1, 3, 4), out["flow"].permute(0, 2, 1, 3, 4)], 1))
        if return_crop:
            dev_out += [out["softmax"].permute(0, 2, 1, 3, 4).contiguous(), out["flow"].permute(0, 2, 1, 3, 4).contiguous(), out["registered"].contiguous()]
        host = self._to_host(dev_out)
        if not want_softmax:
            host[1] = None
        res = tuple(host[:4]) + ((host[4],) if want_raw else (None,))
        if return_crop:
            c = host[-3:]
            return res + ({"softmax": c[0], "flow": c[1], "registered": c[2], "padding_need": pad_need, "size_before": [int(Y), int(X), int(Z)]},)
        return res

    # -- nnUNetTrainer.py:682-726 -> SegFlowGaussian.predict_3D_flow :2837, _internal_predict_2D_2Dconv_tiled_flow :3294-3533
    def predict_preprocessed_data_return_seg_and_softmax_flow(self, unlabeled, target=None, target_mask=None, processor=None,
                                                              do_mirroring=True, mirror_axes=None, use_sliding_window=True, step_size=0.5,
                                                              use_gaussian=True, pad_border_mode="constant", pad_kwargs=None,
                                                              all_in_gpu=False, verbose=True, mixed_precision=True, centroid=None, return_crop=False):
        """unlabeled [T,1,Z,Y,X] (numpy) -> (seg [T,Z,Y,X], softmax [T,K,Z,Y,X], flow [T,2,Z,Y,X], registered [T,1,Z,Y,X],
        raw [T,3,Z,crop,crop]).  target: optional ED label volume [Z,Y,X].  centroid: (x, y) of the heart in the patch, or None (patch
        centre).  return_crop=True appends the crop-space results the voxelmorph_saver layout stores: dict(softmax [T,K,Z,c,c],
        flow [T,2,Z,c,c], registered [T,Z,c,c], padding_need [4,Z], size_before [Y,X,Z])."""
        return self.predict_patients_flow([unlabeled], [target], processor=processor, do_mirroring=do_mirroring, mirror_axes=mirror_axes,
                                          pad_border_mode=pad_border_mode, pad_kwargs=pad_kwargs, centroids=[centroid], return_crop=return_crop)[0]

    def predict_patients_flow(self, unlabeled_list, targets=None, processor=None, do_mirroring=True, mirror_axes=None, pad_border_mode="constant",
                              pad_kwargs=None, centroids=None, return_crop=False, want_raw=True, want_softmax=True):
        """The one-patient call above for several patients whose cropped slices share ONE device batch: every patient is padded / cropped /
        z-scored on its own (`_flow_prepare`), the `[T, Z_p, 1, c, c]` stacks of the patients with the same frame count T are concatenated
        on the slice axis, predict_cine_slices runs once per such group, and each patient's slices go back through its own un-crop
        (`_flow_finish`).  No kernel mixes batch entries; results are those of the one-patient calls up to the launch shapes the batch
        size selects.  Returns one result tuple per patient, in order."""
        if self.flow_net is None:
            raise RuntimeError("this is a segmentation-only model (plans.json has no 'flow_net'): there is no flow route; "
                               "use predict_preprocessed_data_return_seg_and_softmax / predict_volumes_seg")
        processor = processor or self.processor
        mirror_axes = self.data_aug_params["mirror_axes"] if mirror_axes is None else mirror_axes
        n = len(unlabeled_list)
        targets = targets or [None] * n
        centroids = centroids or [None] * n
        prof = API_PROFILE                                  # CF_API_PROFILE=1: synchronise between the stages and add their times to DEVICE_SPLIT
        t0 = time.perf_counter()
        preps = [self._flow_prepare(u, t, processor, pad_border_mode, pad_kwargs, c) for u, t, c in zip(unlabeled_list, targets, centroids)]
        if prof:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            DEVICE_SPLIT["prepare_s"] = DEVICE_SPLIT.get("prepare_s", 0.0) + t1 - t0
        outs = [None] * n
        by_T = {}
        for i, pr in enumerate(preps):
            by_T.setdefault((pr["frames"].shape[0], pr["ed"] is not None), []).append(i)
        for (_T, has_ed), idx in by_T.items():
            frames = preps[idx[0]]["frames"] if len(idx) == 1 else torch.cat([preps[i]["frames"] for i in idx], dim=1)
            ed = None if not has_ed else (preps[idx[0]]["ed"] if len(idx) == 1 else torch.cat([preps[i]["ed"] for i in idx], dim=0))
            out = predict_cine_slices(self.flow_net, self.seg_nets if len(self.seg_nets) > 1 else self.seg_net, frames.contiguous(), ed, do_mirroring, mirror_axes,
                                      seg_mixed_precision=bool(self.mixed_precision and SEG_MIXED_PRECISION))
            z0 = 0
            for i in idx:
                Z = preps[i]["frames"].shape[1]
                outs[i] = {k: v[:, z0:z0 + Z] for k, v in out.items()}
                z0 += Z
        if prof:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            DEVICE_SPLIT["networks_s"] = DEVICE_SPLIT.get("networks_s", 0.0) + t2 - t1
        res = [self._flow_finish(pr, o, return_crop, want_raw, want_softmax) for pr, o in zip(preps, outs)]
        if prof:
            torch.cuda.synchronize()
            DEVICE_SPLIT["finish_s"] = DEVICE_SPLIT.get("finish_s", 0.0) + time.perf_counter() - t2
        return res


# the trainer variants' choices in plans['seg_net'] (nnUNet_variants/architectural_variants): key -> (allowed values or None, default)
SEG_VARIANT_KEYS = {
    "norm": (("in", "gn", "bn", "none"), "in"),
    "norm_groups": (None, 8),
    "nonlin": (("lrelu", "relu", "gelu", "mish"), "lrelu"),
    "nonlin_slope": (None, 0.01),
    "conv_per_stage": (None, 2),
    "block_order": (("conv_norm_nonlin", "conv_nonlin_norm"), "conv_norm_nonlin"),
    "seg_output_bias": ((True, False), False),
}


def _seg_variant_kwargs(sk, arch, flow_net):
    """plans['seg_net'] -> the keyword arguments Generic_UNet / Generic_UNet3D take for a trainer variant ({} for a folder without the
    keys: exactly the stock network).  The keys belong to Generic_UNet alone: next to seg_net.arch or flow_net each is refused, like an
    unknown value, with a ValueError naming both keys."""
    given = [k for k in SEG_VARIANT_KEYS if k in sk]
    for k in given:
        if arch is not None:
            raise ValueError("plans.json holds both seg_net.%s and seg_net.arch == %r: the trainer variants' keys belong to Generic_UNet "
                             "(seg_net.arch absent)" % (k, arch))
        if flow_net:
            raise ValueError("plans.json holds both seg_net.%s and flow_net: the segmentation network next to the flow network is the stock "
                             "Generic_UNet (a trainer variant's folder is segmentation-only)" % k)
        allowed, v = SEG_VARIANT_KEYS[k][0], sk[k]
        if allowed is not None and (v not in allowed or (isinstance(v, bool) != isinstance(allowed[0], bool))):
            raise ValueError("seg_net.%s must be one of %s, got %r" % (k, ", ".join(repr(a) for a in allowed), v))
    def num(k, lo, integer):
        v = sk[k]
        if isinstance(v, bool) or not isinstance(v, (int,) if integer else (int, float)) or not v >= lo:
            raise ValueError("seg_net.%s must be %s >= %s, got %r" % (k, "an integer" if integer else "a number", lo, v))
        return v
    kw = {}
    if "norm" in sk:
        kw["norm"] = sk["norm"]
    if "norm_groups" in sk:
        kw["norm_groups"] = num("norm_groups", 1, True)          # read with norm == 'gn'
    if "nonlin" in sk:
        kw["nonlin"] = sk["nonlin"]
    if "nonlin_slope" in sk:
        kw["nonlin_slope"] = float(num("nonlin_slope", 0.0, False))          # read with nonlin == 'lrelu'
    if "conv_per_stage" in sk:
        kw["num_conv_per_stage"] = num("conv_per_stage", 2, True)
    if "block_order" in sk:
        kw["block_order"] = sk["block_order"]
    if "seg_output_bias" in sk:
        kw["seg_output_bias"] = sk["seg_output_bias"]
    return kw


def _check_regions(plans, arch, flow_net):
    """plans['seg_net']['regions'] / ['regions_class_order'] (region-based training, nnUNetTrainerV2BraTSRegions*: one sigmoid channel per
    region, labels painted in regions_class_order) -> (regions as an ordered {name: [labels]}, [label per region]), or (None, None) for a
    folder without either key.  Everything the two keys must not stand next to is refused here, before a network is built."""
    sk = plans.get("seg_net") or {}
    has_r, has_o = sk.get("regions") is not None, sk.get("regions_class_order") is not None
    if not has_r and not has_o:
        return None, None
    if has_r != has_o:
        raise ValueError("plans.json holds seg_net.%s without seg_net.%s: a region-based folder needs both seg_net.regions and "
                         "seg_net.regions_class_order" % (("regions", "regions_class_order") if has_r else ("regions_class_order", "regions")))
    if flow_net:
        raise ValueError("plans.json holds both seg_net.regions and flow_net: label propagation one-hot encodes exclusive labels (a "
                         "region-based folder is segmentation-only)")
    if arch == "mtl":
        raise ValueError("plans.json holds both seg_net.regions and seg_net.arch == 'mtl': MTLmodel has no region-based trainer")
    if sk.get("prev_stage_classes") is not None:
        raise ValueError("plans.json holds both seg_net.regions and seg_net.prev_stage_classes: a cascade stage takes and gives exclusive labels")
    regions, order = sk["regions"], sk["regions_class_order"]
    is_label = lambda c: isinstance(c, int) and not isinstance(c, bool) and 0 <= c <= 255     # noqa: E731
    if not isinstance(regions, dict) or not regions:
        raise ValueError("seg_net.regions must be a non-empty mapping from region name to a list of label values, got %r" % (regions,))
    for name, labels in regions.items():
        if not isinstance(labels, (list, tuple)) or not labels:
            raise ValueError("seg_net.regions[%r] is an empty region: every region is a non-empty list of label values, got %r" % (name, labels))
        if not all(is_label(c) for c in labels):
            raise ValueError("seg_net.regions[%r] holds a label outside 0..255: %r" % (name, labels))
    if not isinstance(order, (list, tuple)) or not all(is_label(c) for c in order):
        raise ValueError("seg_net.regions_class_order must be a list of label values in 0..255, got %r" % (order,))
    if len(order) != len(regions):
        raise ValueError("seg_net.regions_class_order has %d entries and seg_net.regions has %d: one label per region" % (len(order), len(regions)))
    if plans["num_classes"] != len(regions):
        raise ValueError("plans.json holds num_classes == %r next to %d seg_net.regions: a region-based network has one sigmoid channel per "
                         "region and no background channel, so num_classes must equal len(seg_net.regions)" % (plans["num_classes"], len(regions)))
    return {str(k): [int(c) for c in v] for k, v in regions.items()}, [int(c) for c in order]


def _check_mtl_plans(plans, seg_dim, flow_net):
    """plans['seg_net']['arch'] == 'mtl' (the segmenter nnMTLTrainerV2 trains): what the plans must not hold next to it"""
    sk = plans["seg_net"]
    if seg_dim != 2:
        raise ValueError("plans.json holds seg_net.arch == 'mtl' with seg_net.dim == %d: MTLmodel is a 2-D network" % seg_dim)
    if flow_net:
        raise ValueError("plans.json holds both seg_net.arch == 'mtl' and flow_net: MTLmodel next to the flow network is not built (an "
                         "MTLmodel folder is segmentation-only)")
    if sk.get("prev_stage_classes") is not None:
        raise ValueError("plans.json holds both seg_net.arch == 'mtl' and seg_net.prev_stage_classes: the reference has no cascade trainer "
                         "for MTLmodel")
    if "image_size" not in plans or list(plans["patch_size"]) != [plans["image_size"], plans["image_size"]]:
        raise ValueError("seg_net.arch == 'mtl' needs patch_size == [image_size, image_size] (nnMTLTrainerV2 predicts on the whole "
                         "image_size square), got patch_size %r and image_size %r" % (plans["patch_size"], plans.get("image_size")))
    if plans.get("cropping_net") and "crop_size" not in plans:
        raise ValueError("plans.json holds seg_net.arch == 'mtl' and cropping_net without crop_size: the segmenter runs on the crop_size "
                         "window the cropping network centres")
    for key in ("config", "window_size"):
        if key not in sk:
            raise ValueError("seg_net.arch == 'mtl' needs seg_net.%s" % key)


def _check_prev_stage(prev_stage_classes, given, model_folder):
    if prev_stage_classes and not given:
        raise ValueError("the model%s is the full-resolution stage of a cascade (seg_net.prev_stage_classes = %r): it needs the previous stage's "
                         "segmentations (-l / lowres_segmentations / segs_from_prev_stage, or --lowres_model)"
                         % (" in %s" % model_folder if model_folder else "", list(prev_stage_classes)))
    if given and not prev_stage_classes:
        raise ValueError("segmentations from a previous stage were given (-l), but the model%s has no seg_net.prev_stage_classes in its plans.json: "
                         "it is not a cascade stage and would ignore them" % (" in %s" % model_folder if model_folder else ""))


def _fold_dirs(folder, folds):
    if folds is None or folds == "None":
        return sorted(d for d in os.listdir(folder) if d.startswith("fold_"))
    if isinstance(folds, (list, tuple)):
        return ["fold_%s" % i if str(i) != "all" else "all" for i in folds]
    return ["fold_%s" % folds]


_CHECKPOINT_PARTS = (("seg_state_dict", "seg_net"), ("flow_state_dict", "flow_net"), ("crop_state_dict", "crop_net"))


def _broadcast_params(trainer, params, nfolds, device):
    """The one collective of the multi-GPU path (the reference has no hook: every `--part_id` process of
    predict.py:806-821 reads the checkpoint itself): rank 0 holds `params` (the folds' checkpoint dicts), every rank gets each fold's weights
    as ONE flat fp32 broadcast (RCCL over xGMI under the nccl backend, gloo on CPU tensors) and rebuilds the dicts `load_checkpoint_ram` takes.
    Shapes come from the networks every rank built from plans.json, so ranks >= 1 need no checkpoint file."""
    shapes = {}
    for key, attr in _CHECKPOINT_PARTS:
        net = getattr(trainer, attr, None)
        if net is not None:
            for k, v in net.state_shapes().items():
                if not k.endswith("grid"):                                       # SpatialTransformer grids are rebuilt, never loaded
                    shapes[key + "/" + k] = v
    rank = dist.get_rank()
    out = []
    for f in range(nfolds):
        flat = None
        if rank == 0:
            flat = {}
            for key, _ in _CHECKPOINT_PARTS:
                for k, v in (params[f].get(key) or {}).items():
                    if key + "/" + k in shapes:
                        flat[key + "/" + k] = v
            missing = sorted(set(shapes) - set(flat))
            if missing:
                raise KeyError("checkpoint lacks %d tensors the networks of plans.json need, e.g. %s" % (len(missing), missing[:3]))
        got = parallel.broadcast_state_dict(flat, shapes, device)
        p = {}
        for name, t in got.items():
            key, k = name.split("/", 1)
            p.setdefault(key, {})[k] = t
        out.append(p)
    return out


def load_model_and_checkpoint_files(folder, folds=None, mixed_precision=None, checkpoint_name="model_final_checkpoint", device=None):
    """model_restore.py:109-155 equivalent for the plans.json / *.model folder format -> (trainer, [params per fold]).
    In a multi-process job (WORLD_SIZE > 1, one process per GPU) only rank 0 reads `fold_X/<checkpoint_name>.model`; the other ranks need
    plans.json alone and receive the weights through cineflow.parallel.broadcast_state_dict before the patient loop."""
    assert os.path.isfile(join(folder, "plans.json")), "Folder with saved model weights must contain a plans.json file"
    with open(join(folder, "plans.json")) as f:
        plans = json.load(f)
    device = device or torch.device("cuda", torch.cuda.current_device())
    trainer = CineTrainer(plans, device, model_folder=folder)
    trainer.mixed_precision = bool(mixed_precision)
    rank, world, _ = parallel.init_from_env()
    if world > 1:
        fold_dirs = _fold_dirs(folder, folds) if rank == 0 else None
        n = torch.tensor([len(fold_dirs) if rank == 0 else 0], dtype=torch.int64, device=device if device.type == "cuda" else "cpu")
        dist.broadcast(n, src=0)
        params = ([torch.load(join(folder, f, checkpoint_name + ".model"), map_location="cpu", weights_only=True) for f in fold_dirs]
                  if rank == 0 else None)
        return trainer, _broadcast_params(trainer, params, int(n.item()), device)
    params = [torch.load(join(folder, f, checkpoint_name + ".model"), map_location="cpu", weights_only=True) for f in _fold_dirs(folder, folds)]
    return trainer, params

# ------------------------------------------------------------------------------------------------ model cache
_MODEL_CACHE = {}


def clear_model_cache():
    """drop the resident model of `_cached_model` (the next predict_* call reads plans.json and the checkpoint again)"""
    _MODEL_CACHE.clear()


def _file_stamp(path):
    try:
        st = os.stat(path)
        return (st.st_mtime_ns, st.st_size)
    except OSError:
        return None


def _model_stamp(model, folds, checkpoint_name):
    """(mtime_ns, size) of plans.json, of every selected fold's <checkpoint_name>.model and of the config files plans.json may name: a
    checkpoint rewritten in place (same plans) must not be served from the cache.  Ranks without checkpoint files stamp what they have."""
    stamp = [_file_stamp(join(model, "plans.json"))]
    try:
        fold_dirs = _fold_dirs(model, folds)
    except OSError:
        fold_dirs = []
    for f in fold_dirs:
        stamp.append((f, _file_stamp(join(model, f, checkpoint_name + ".model"))))
    for extra in sorted(glob.glob(join(model, "*.yaml"))):
        stamp.append((os.path.basename(extra), _file_stamp(extra)))
    return tuple(stamp)


def _cached_model(model, folds, mixed_precision, checkpoint_name):
    """load_model_and_checkpoint_files + load_ensemble (every selected fold) once per (folder, folds, checkpoint, mixed_precision, device, the CF_* knobs in
    force) and per state of the files on disk (`_model_stamp`): predict_from_folder used to rebuild both networks and re-read the checkpoint
    for every patient.  The reference re-reads the checkpoint on every predict_cases call; `clear_model_cache()` forces that here."""
    knobs = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("CF_")))
    key = (os.path.abspath(model), str(folds), checkpoint_name, bool(mixed_precision), torch.cuda.current_device(), knobs)
    stamp = _model_stamp(model, folds, checkpoint_name)
    hit = _MODEL_CACHE.get(key)
    if hit is None or hit[0] != stamp:
        _MODEL_CACHE.clear()                                                     # one model resident at a time
        trainer, params = load_model_and_checkpoint_files(model, folds, mixed_precision=mixed_precision, checkpoint_name=checkpoint_name)
        trainer.load_ensemble(params)                                            # every selected fold resident, packed once
        trainer._ensemble_of = params
        hit = (stamp, trainer, params)
        _MODEL_CACHE[key] = hit
    return hit[1], hit[2]
