"""Import of a model folder written by the reference's nnUNetTrainerV2_ResencUNet (cineflow.reference_models), host side: the residual
planner's plans translation, the importer's dispatch and its check against FabiansUNet3D, the decoder tensors the reference registers
twice, and every refusal -- each before anything is written.

The fixture tree tests/golden/ref_model_folder_resenc/ was written by the reference's own save_checkpoint
(make_golden_refckpt_resenc.py)."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RESENC = os.path.join(HERE, "golden", "ref_model_folder_resenc")
FLOW = os.path.join(HERE, "golden", "ref_model_folder", "flow")
POOL, KERN = [[1, 1, 1], [1, 2, 2], [2, 2, 2]], [[1, 3, 3], [3, 3, 3], [3, 3, 3]]
CHK = os.path.join("fold_0", "model_final_checkpoint.model")


def _R():
    from cineflow import reference_models
    return reference_models


def _plans():
    return _R().load_reference_pickle(os.path.join(RESENC, "plans.pkl"))


def _with_stage(plans, **kw):
    return dict(plans, plans_per_stage={0: dict(plans["plans_per_stage"][0], **kw)})


def _rewrite_checkpoint(path, edit):
    """load a reference checkpoint in full (the numpy globals admitted), change its state_dict, write it back in the same layout"""
    R = _R()
    with torch.serialization.safe_globals(R._numpy_safe_globals()):
        ck = torch.load(path, map_location="cpu", weights_only=True)
    edit(ck["state_dict"])
    torch.save(ck, path)


def _copy(tmp_path):
    seg = str(tmp_path / "resenc")
    shutil.copytree(RESENC, seg)
    return seg


def test_plans_translation_of_the_resenc_fixture():
    R = _R()
    plans = _plans()
    stage = plans["plans_per_stage"][0]
    assert tuple(stage["num_blocks_encoder"]) == (1, 2, 3) and tuple(stage["num_blocks_decoder"]) == (1, 1)
    assert len(stage["pool_op_kernel_sizes"]) == len(stage["conv_kernel_sizes"]) == 3
    p = R.plans_from_reference_3d(plans)
    assert p["num_classes"] == 4 and p["num_modalities"] == 1
    assert p["patch_size"] == [8, 32, 32] and p["mirror_axes"] == [0, 1, 2]
    assert p["seg_net"] == {"dim": 3, "arch": "resenc", "base_num_features": 4, "num_pool": 2, "pool_op_kernel_sizes": POOL,
                            "conv_kernel_sizes": KERN, "num_blocks_encoder": [1, 2, 3], "num_blocks_decoder": [1, 1]}
    assert p["preprocessor_name"] == "GenericPreprocessor" and p["stage"] == 0
    assert "flow_net" not in p and "crop_size" not in p
    assert json.loads(json.dumps(p)) == p                                            # plain JSON values only


def test_resenc_refusals_name_their_key():
    R = _R()
    plans = _plans()
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):           # no leading [1, 1, 1]
        R.plans_from_reference_3d(_with_stage(plans, pool_op_kernel_sizes=[[1, 2, 2], [1, 2, 2], [2, 2, 2]]))
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):
        R.plans_from_reference_3d(_with_stage(plans, pool_op_kernel_sizes=[[1, 1, 1], [1, 2, 2], [3, 2, 2]]))
    with pytest.raises(NotImplementedError, match="pool_op_kernel_sizes"):           # unequal in-plane
        R.plans_from_reference_3d(_with_stage(plans, pool_op_kernel_sizes=[[1, 1, 1], [1, 2, 1], [2, 2, 2]]))
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):              # one kernel more than pooling entries: the plain layout
        R.plans_from_reference_3d(_with_stage(plans, conv_kernel_sizes=KERN + [[3, 3, 3]]))
    with pytest.raises(NotImplementedError, match="conv_kernel_sizes"):
        R.plans_from_reference_3d(_with_stage(plans, conv_kernel_sizes=[[1, 3, 3], [3, 3, 3], [5, 3, 3]]))
    with pytest.raises(NotImplementedError, match="num_blocks_encoder"):
        R.plans_from_reference_3d(_with_stage(plans, num_blocks_encoder=(1, 2)))
    with pytest.raises(NotImplementedError, match="num_blocks_decoder"):
        R.plans_from_reference_3d(_with_stage(plans, num_blocks_decoder=(1, 1, 1)))
    stage = {k: v for k, v in plans["plans_per_stage"][0].items() if k != "num_blocks_decoder"}
    with pytest.raises(NotImplementedError, match="num_blocks_decoder"):           # the reference's trainer reads it unconditionally
        R.plans_from_reference_3d(dict(plans, plans_per_stage={0: stage}))


def test_import_builds_the_residual_encoder_unet_with_the_reference_shapes(tmp_path):
    R = _R()
    from cineflow.models import FabiansUNet3D
    from cineflow.predict import CineTrainer
    out = str(tmp_path / "out")
    plans_written = R.import_reference_model_folder(RESENC, None, out)
    with open(os.path.join(out, "plans.json")) as f:
        plans = json.load(f)
    assert plans == json.loads(json.dumps(plans_written))
    assert plans["seg_net"]["arch"] == "resenc" and plans["seg_net"]["dim"] == 3 and "flow_net" not in plans
    trainer = CineTrainer(plans, torch.device("cpu"), model_folder=out)
    assert isinstance(trainer.seg_net, FabiansUNet3D) and trainer.flow_net is None and trainer.processor is None
    ck = torch.load(os.path.join(out, CHK), map_location="cpu", weights_only=True)
    assert set(ck) == {"seg_state_dict"}
    shapes = trainer.seg_net.state_shapes()
    assert {k: tuple(v.shape) for k, v in ck["seg_state_dict"].items()} == shapes
    assert not any(".all." in k for k in shapes)
    assert shapes["encoder.initial_conv.weight"] == (4, 1, 3, 3, 3)
    assert shapes["encoder.stages.0.convs.0.conv1.weight"] == (4, 4, 1, 3, 3)
    assert not any(k.startswith("encoder.stages.0.") and "downsample_skip" in k for k in shapes)      # stride [1,1,1], 4 -> 4: identity skip
    assert shapes["encoder.stages.1.convs.0.downsample_skip.0.weight"] == (8, 4, 1, 1, 1)
    assert "encoder.stages.1.convs.0.downsample_skip.0.bias" not in shapes
    assert shapes["encoder.stages.1.convs.0.downsample_skip.1.bias"] == (8,)
    assert "encoder.stages.1.convs.1.downsample_skip.0.weight" not in shapes
    assert shapes["encoder.stages.2.convs.2.conv2.weight"] == (16, 16, 3, 3, 3)
    assert shapes["decoder.tus.0.weight"] == (16, 8, 2, 2, 2) and shapes["decoder.tus.1.weight"] == (8, 4, 1, 2, 2)
    assert shapes["decoder.stages.0.convs.0.conv.weight"] == (8, 16, 3, 3, 3)
    assert shapes["decoder.stages.1.convs.0.conv.weight"] == (4, 8, 1, 3, 3)
    assert shapes["decoder.segmentation_output.weight"] == (4, 4, 1, 1, 1)
    assert shapes["decoder.deep_supervision_outputs.0.weight"] == (4, 8, 1, 1, 1)
    # the imported tensors are the reference's, bit for bit
    ref = R.load_reference_checkpoint(os.path.join(RESENC, CHK))["state_dict"]
    assert all(torch.equal(ck["seg_state_dict"][k], ref[k]) for k in shapes)
    # the reference registers every decoder conv / norm twice; the fixture really has the aliases
    assert torch.equal(ref["decoder.stages.0.convs.0.all.0.weight"], ref["decoder.stages.0.convs.0.conv.weight"])
    assert "decoder.stages.1.convs.0.all.2.bias" in ref


def test_the_command_line_imports_the_folder(tmp_path):
    out = str(tmp_path / "out")
    _R().main(["-s", RESENC, "-o", out])
    with open(os.path.join(out, "plans.json")) as f:
        assert json.load(f)["seg_net"]["arch"] == "resenc"


@pytest.mark.parametrize("what", ["alias_unequal", "alias_missing", "skip_norm_bias_missing", "conv2_reshaped", "batchnorm"])
def test_a_wrong_checkpoint_fails_the_import_before_anything_is_written(tmp_path, what):
    R = _R()
    seg = _copy(tmp_path)

    def edit(sd):
        if what == "alias_unequal":
            k = "module.decoder.stages.1.convs.0.all.0.weight"
            sd[k] = sd[k].clone()
            sd[k].view(-1)[3] += 1e-3
        elif what == "alias_missing":
            del sd["module.decoder.stages.0.convs.0.all.2.bias"]
        elif what == "skip_norm_bias_missing":
            del sd["module.encoder.stages.1.convs.0.downsample_skip.1.bias"]
        elif what == "conv2_reshaped":
            k = "module.encoder.stages.1.convs.0.conv2.weight"
            sd[k] = sd[k][:, :, :1].contiguous()                                      # (8, 8, 1, 3, 3) where the plans say (3,3,3)
        else:
            sd["module.encoder.initial_norm.running_mean"] = torch.zeros(4)
            sd["module.encoder.initial_norm.running_var"] = torch.ones(4)
    _rewrite_checkpoint(os.path.join(seg, CHK), edit)
    exc, match = {"alias_unequal": (ValueError, r"decoder\.stages\.1\.convs\.0\.all\.0\.weight"),
                  "alias_missing": (ValueError, r"decoder\.stages\.0\.convs\.0\.(all\.2|norm)\.bias"),
                  "skip_norm_bias_missing": (KeyError, r"downsample_skip\.1\.bias"),
                  "conv2_reshaped": (ValueError, r"encoder\.stages\.1\.convs\.0\.conv2\.weight"),
                  "batchnorm": (NotImplementedError, "norm_type='bn'")}[what]
    with pytest.raises(exc, match=match):
        R.import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def _rename_trainer(seg, name):
    p = os.path.join(seg, CHK + ".pkl")
    info = _R().load_reference_pickle(p)
    info["name"] = name
    info["class"] = str(info["class"])
    with open(p, "wb") as f:
        pickle.dump(info, f)


def test_a_bn_trainer_is_refused(tmp_path):
    seg = _copy(tmp_path)
    _rename_trainer(seg, "nnUNetTrainerV2_ResencUNet_DA3_BN")
    with pytest.raises(NotImplementedError, match="norm_type='bn'"):
        _R().import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_name_and_plans_must_agree(tmp_path):
    R = _R()
    seg = _copy(tmp_path)
    _rename_trainer(seg, "nnUNetTrainerV2")
    with pytest.raises(ValueError, match="nnUNetTrainerV2.*num_blocks_encoder"):
        R.import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
    # ... and the other way round: a ResencUNet trainer's name on plans without num_blocks_encoder
    seg3d = str(tmp_path / "seg3d")
    shutil.copytree(os.path.join(HERE, "golden", "ref_model_folder_3d"), seg3d)
    _rename_trainer(seg3d, "nnUNetTrainerV2_ResencUNet")
    with pytest.raises(ValueError, match="ResencUNet.*num_blocks_encoder"):
        R.import_reference_model_folder(seg3d, None, str(tmp_path / "out2"))
    assert not (tmp_path / "out2").exists()


def test_the_da3_variant_is_the_same_network(tmp_path):
    seg = _copy(tmp_path)
    _rename_trainer(seg, "nnUNetTrainerV2_ResencUNet_DA3")
    p = _R().import_reference_model_folder(seg, None, str(tmp_path / "out"))
    assert p["seg_net"]["arch"] == "resenc"


def test_a_resenc_folder_with_a_flow_folder_is_refused(tmp_path):
    with pytest.raises(ValueError, match="flow path is 2-D"):
        _R().main(["-s", RESENC, "-w", FLOW, "-o", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()


def test_arch_resenc_is_refused_outside_3d_segmentation_only_plans():
    from cineflow.predict import CineTrainer
    good = _R().plans_from_reference_3d(_plans())
    CineTrainer(good, torch.device("cpu"))
    p = json.loads(json.dumps(good))
    p["seg_net"]["dim"] = 2
    p["patch_size"] = [32, 32]
    with pytest.raises(ValueError, match=r"arch.*dim|dim.*arch"):
        CineTrainer(p, torch.device("cpu"))
    p = json.loads(json.dumps(good))
    del p["seg_net"]["dim"]                                                          # dim defaults to 2
    p["patch_size"] = [32, 32]
    with pytest.raises(ValueError, match=r"arch.*dim|dim.*arch"):
        CineTrainer(p, torch.device("cpu"))
    p = json.loads(json.dumps(good))
    p["seg_net"]["prev_stage_classes"] = [1, 2, 3]
    with pytest.raises(ValueError, match=r"arch.*prev_stage_classes|prev_stage_classes.*arch"):
        CineTrainer(p, torch.device("cpu"))
    p = json.loads(json.dumps(good))
    p["seg_net"]["arch"] = "preact"
    with pytest.raises(ValueError, match="arch"):
        CineTrainer(p, torch.device("cpu"))


def test_arch_resenc_with_a_flow_net_names_both_keys():
    from cineflow.predict import CineTrainer
    p = _R().plans_from_reference_3d(_plans())
    p["flow_net"] = {"variant": "video", "kwargs": {}}
    p["crop_size"] = 32
    with pytest.raises(ValueError, match=r"arch.*flow_net"):
        CineTrainer(p, torch.device("cpu"))


def test_plans_without_num_blocks_encoder_take_the_plain_rule():
    R = _R()
    plans = _plans()
    stage = {k: v for k, v in plans["plans_per_stage"][0].items() if k not in ("num_blocks_encoder", "num_blocks_decoder")}
    stage["pool_op_kernel_sizes"] = POOL[1:]
    p = R.plans_from_reference_3d(dict(plans, plans_per_stage={0: stage}))
    assert "arch" not in p["seg_net"] and p["seg_net"]["num_pool"] == 2 and p["seg_net"]["pool_op_kernel_sizes"] == POOL[1:]
    assert isinstance(np.asarray(stage["patch_size"]), np.ndarray)
