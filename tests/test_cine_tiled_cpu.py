"""CPU tests (no GPU) of the cine-batched sliding window's entry points, of segmentation-only model folders and of fold ensembles:
argument validation of cf_tile_gather / cf_tile_merge, the plans.json / checkpoint round trip of a folder without a flow network,
the importer without a flow folder, and the world-size-2 weight broadcast of a segmentation-only two-fold ensemble."""
import ctypes
import json
import os
import shutil
import socket

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.join(HERE, "golden", "ref_model_folder")


def _ints(*v):
    a = (ctypes.c_int * len(v))(*v)
    return a, ctypes.cast(a, ctypes.c_void_p)


def test_tile_gather_and_merge_reject_bad_arguments_without_a_device():
    """every argument error is caught on the host (CF_ERR_ARG = -1 and a message); the non-null pointers are never dereferenced"""
    from cineflow import _lib
    h = _lib.lib()
    p = 4096                                                                      # a non-null, 16-byte aligned address that is never touched
    assert h.cf_tile_gather(None, p, p, 1, 1, 1, 8, 8, 4, 4, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tile_gather(p, None, p, 1, 1, 1, 8, 8, 4, 4, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tile_gather(p, p, p, 0, 1, 1, 8, 8, 4, 4, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_tile_gather(p, p, p, 1, 1, 1, 8, 8, 9, 4, None) == -1 and b"bad shape" in h.cf_last_error()          # patch larger than the image
    assert h.cf_tile_gather(p, p, p, 1, 1, 1, 8, 8, 4, 0, None) == -1
    keep, lx = _ints(0, 4)
    keep1, one = _ints(0)
    assert h.cf_tile_merge(None, None, p, p, 1, 4, 8, 8, 4, 4, lx, 2, lx, 2, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, None, 2, lx, 2, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_tile_merge(p, None, p, p, 1, 0, 8, 8, 4, 4, lx, 2, lx, 2, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_tile_merge(p, None, p, p, 1, 256, 8, 8, 4, 4, lx, 2, lx, 2, None) == -1                                # seg is uint8
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, lx, 17, lx, 2, None) == -1 and b"1..16 steps" in h.cf_last_error()
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, lx, 0, lx, 2, None) == -1
    keep2, gap = _ints(0, 5)                                                      # 0..4 and 5..9 on an axis of 8: leaves the image
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, gap, 2, lx, 2, None) == -1 and b"step lists" in h.cf_last_error()
    keep3, hole = _ints(0, 6)                                                     # patch 4 on an axis of 10: rows 4, 5 uncovered
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 10, 8, 4, 4, hole, 2, lx, 2, None) == -1 and b"step lists" in h.cf_last_error()
    keep4, down = _ints(4, 0)
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, down, 2, lx, 2, None) == -1
    assert h.cf_tile_merge(p, None, p, p, 1, 4, 8, 8, 4, 4, one, 1, lx, 2, None) == -1                                 # one window of 4 does not span 8


def test_ops_wrappers_reject_host_tensors():
    from cineflow import ops
    with pytest.raises(TypeError):
        ops.tile_gather(torch.zeros(1, 1, 8, 8), torch.zeros(1, 3, dtype=torch.int32), 4, 4)
    with pytest.raises(TypeError):
        ops.tile_merge(torch.zeros(4, 2, 4, 4), None, 8, 8, [0, 4], [0, 4])


def _seg_only_folder(folder, seeds=(10, 20)):
    from cineflow import predict as P
    from cineflow.models import Generic_UNet
    from cineflow.weights import seeded_state_dict
    plans = P.default_plans(image_size=64, flow_variant=None, seg_base=8, seg_pool=3)
    seg = Generic_UNet(1, 8, 4, 3)
    sds = [seeded_state_dict(seg.state_shapes(), s) for s in seeds]
    for f, sd in enumerate(sds):
        P.save_model_folder(folder, seg, None, plans, fold=f, seg_sd=sd, flow_sd=None)
    return plans, sds


def test_segmentation_only_plans_round_trip_on_cpu(tmp_path):
    """default_plans(flow_variant=None) -> save_model_folder(folder, seg_net, None, ...) -> load_model_and_checkpoint_files: no flow network,
    no Processor, no 'flow_state_dict'; load_ensemble keeps every fold resident and load_checkpoint_ram goes back to one fold."""
    from cineflow import predict as P
    folder = str(tmp_path / "model")
    plans, sds = _seg_only_folder(folder)
    assert "flow_net" not in plans and "crop_size" not in plans
    with open(os.path.join(folder, "plans.json")) as f:
        assert json.load(f) == plans
    trainer, params = P.load_model_and_checkpoint_files(folder, None, device=torch.device("cpu"))
    assert trainer.flow_net is None and trainer.processor is None and trainer.crop_net is None
    assert len(params) == 2 and all(sorted(p) == ["seg_state_dict"] for p in params)
    for p, sd in zip(params, sds):
        assert sorted(p["seg_state_dict"]) == sorted(sd) and all(torch.equal(p["seg_state_dict"][k], sd[k]) for k in sd)
    trainer.load_ensemble(params)
    assert len(trainer.seg_nets) == 2 and trainer.seg_nets[0] is trainer.seg_net and trainer.seg_nets[1] is not trainer.seg_net
    trainer.load_checkpoint_ram(params[1])
    assert trainer.seg_nets == [trainer.seg_net]
    # "flow_net": null means the same as no entry
    with open(os.path.join(folder, "plans.json"), "w") as f:
        json.dump(dict(plans, flow_net=None), f)
    trainer, _ = P.load_model_and_checkpoint_files(folder, [0], device=torch.device("cpu"))
    assert trainer.flow_net is None
    with pytest.raises(RuntimeError, match="segmentation-only"):
        trainer.predict_patients_flow([])
    # a flow model still refuses a checkpoint without its flow weights
    red = dict(in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32], d_model=32, bottleneck_heads=4, dim_feedforward=48)
    tr = P.CineTrainer(P.default_plans(image_size=64, crop_size=64, seg_base=8, seg_pool=3, reduced=red), torch.device("cpu"))
    with pytest.raises(KeyError, match="flow_state_dict"):
        tr.load_checkpoint_ram({"seg_state_dict": sds[0]})


def test_import_reference_segmentation_folder_on_its_own(tmp_path):
    """import_reference_model_folder(seg, None, out) / the CLI without -w: a segmentation-only folder with every check of the segmentation side"""
    from cineflow import predict as P
    from cineflow import reference_models as R
    out = str(tmp_path / "out")
    plans = R.import_reference_model_folder(os.path.join(TREE, "seg"), None, out)
    assert "flow_net" not in plans and "crop_size" not in plans and plans["patch_size"] == [64, 64] and plans["num_classes"] == 4
    assert sorted(os.listdir(out)) == ["fold_0", "plans.json"]
    trainer, params = P.load_model_and_checkpoint_files(out, None, device=torch.device("cpu"))
    assert trainer.flow_net is None and sorted(params[0]) == ["seg_state_dict"]
    want = R.load_reference_checkpoint(os.path.join(TREE, "seg", "fold_0", "model_final_checkpoint.model"))["state_dict"]
    assert all(torch.equal(params[0]["seg_state_dict"][k], want[k]) for k in params[0]["seg_state_dict"])
    out2 = str(tmp_path / "out2")
    R.main(["-s", os.path.join(TREE, "seg"), "-o", out2])
    assert sorted(os.listdir(out2)) == ["fold_0", "plans.json"]
    with pytest.raises(ValueError, match="crop_size"):
        R.import_reference_model_folder(os.path.join(TREE, "seg"), None, str(tmp_path / "x"), crop_size=64)
    with pytest.raises(FileNotFoundError, match="fold_3"):
        R.import_reference_model_folder(os.path.join(TREE, "seg"), None, str(tmp_path / "x"), folds=[3])
    # the segmentation side's tensor check still bites: a checkpoint that lacks a tensor is refused before anything is written
    bad = tmp_path / "bad_seg"
    shutil.copytree(os.path.join(TREE, "seg"), str(bad))
    ck_path = str(bad / "fold_0" / "model_final_checkpoint.model")
    with torch.serialization.safe_globals(R._numpy_safe_globals()):
        ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    ck["state_dict"].pop(sorted(ck["state_dict"])[0])
    torch.save(ck, ck_path)
    with pytest.raises(KeyError, match="lacks 1 tensors"):
        R.import_reference_model_folder(str(bad), None, str(tmp_path / "y"))
    assert not os.path.exists(str(tmp_path / "y"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ensemble_worker(rank, world, port, q, folders):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "cardiac-segmentation-optical-flow_amd"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from cineflow import parallel, predict
    parallel.init_from_env(backend="gloo")
    trainer, params = predict.load_model_and_checkpoint_files(folders[rank], folds=None, mixed_precision=True, device=torch.device("cpu"))
    trainer.load_ensemble(params)
    sums = [(sorted(p), len(p["seg_state_dict"]), float(sum(float(v.double().sum()) for v in p["seg_state_dict"].values()))) for p in params]
    parallel.barrier()
    q.put((rank, sums, len(trainer.seg_nets), trainer.flow_net is None))
    torch.distributed.destroy_process_group()


def test_segmentation_only_two_fold_ensemble_broadcast_two_ranks(tmp_path):
    """rank 0 reads fold_0 and fold_1 of a segmentation-only folder; rank 1 holds plans.json only and receives both folds"""
    f0, f1 = str(tmp_path / "rank0"), str(tmp_path / "rank1")
    _plans, sds = _seg_only_folder(f0, seeds=(3, 4))
    os.makedirs(f1)
    shutil.copy(os.path.join(f0, "plans.json"), f1)
    assert sorted(os.listdir(f1)) == ["plans.json"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ensemble_worker, args=(r, 2, port, q, [f0, f1])) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = [float(sum(float(v.double().sum()) for v in sd.values())) for sd in sds]
    assert abs(want[0] - want[1]) > 1e-3                                          # the folds differ: a rank that got fold 0 twice would show
    for _rank, sums, nnets, seg_only in res:
        assert nnets == 2 and seg_only and len(sums) == 2
        for (keys, n, total), sd, w in zip(sums, sds, want):
            assert keys == ["seg_state_dict"] and n == len(sd) and abs(total - w) < 1e-6 * (1 + abs(w))
