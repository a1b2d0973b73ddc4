"""cineflow.experiment_planning on the host (no GPU): every plans entry of every planner-only fixture equals what the reference's planners
wrote (tests/golden/make_golden_plan_and_preprocess.py), the written pickles are plain data the importers accept, unknown planner names
raise, and the count / select entries of csrc/dataset.hip refuse bad arguments before any launch."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from _plan_compare import assert_same, relative_paths

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "plan_and_preprocess", "planner_only.pkl")


@pytest.fixture(scope="module")
def planner_only():
    from cineflow.safe_pickle import load_plain_pickle
    return load_plain_pickle(FIXTURE)


def _folders(tmp_path, name, fx):
    """a cropped folder as far as a planner reads it: dataset_properties.pkl, the case list (.npz names) and each case's .pkl"""
    cropped, pre = str(tmp_path / ("cropped_" + name)), str(tmp_path / ("planned_" + name))
    os.makedirs(cropped)
    os.makedirs(pre)
    with open(os.path.join(cropped, "dataset_properties.pkl"), "wb") as f:
        pickle.dump(fx["dataset_properties"], f)
    for c in fx["cases"]:
        open(os.path.join(cropped, c + ".npz"), "wb").close()
        with open(os.path.join(cropped, c + ".pkl"), "wb") as f:
            pickle.dump({}, f)
    return cropped, pre


def _plan(tmp_path, name, fx, planner):
    from cineflow import experiment_planning as EP
    from cineflow.safe_pickle import load_plain_pickle
    cropped, pre = _folders(tmp_path / planner, name, fx)
    cls = EP.find_planner(planner)
    p = cls(cropped, pre, fx["config"]) if planner == "CustomExperimentPlanner" else cls(cropped, pre)
    p.plan_experiment()
    return p, load_plain_pickle(p.plans_fname), cropped


CASES = [("lowres", "ExperimentPlanner"), ("lowres", "ExperimentPlanner3D_v21"), ("lowres", "ExperimentPlanner2D"), ("lowres", "ExperimentPlanner2D_v21"),
         ("shrink2d", "ExperimentPlanner3D_v21"), ("shrink2d", "ExperimentPlanner2D_v21"),
         ("custom", "CustomExperimentPlanner"), ("custom", "ExperimentPlanner2D"), ("custom", "ExperimentPlanner2D_v21"), ("custom", "ExperimentPlanner"),
         ("custom", "ExperimentPlanner3D_v21")]


def test_fixture_lists_the_cases_tested_here(planner_only):
    assert sorted((s, p) for s, fx in planner_only.items() for p in fx["plans"]) == sorted(CASES)


@pytest.mark.parametrize("name,planner", CASES)
def test_plans_equal_the_reference(tmp_path, planner_only, name, planner):
    fx = planner_only[name]
    p, plans, cropped = _plan(tmp_path, name, fx, planner)
    want = fx["plans"][planner]
    assert list(plans.keys()) == list(want.keys())
    assert_same(relative_paths(plans, str(tmp_path / planner)), want, planner)
    assert os.path.basename(p.plans_fname) == {"ExperimentPlanner": "nnUNetPlansfixed_plans_3D.pkl", "ExperimentPlanner3D_v21": "nnUNetPlansv2.1_plans_3D.pkl",
                                               "ExperimentPlanner2D": "nnUNetPlans_plans_2D.pkl", "ExperimentPlanner2D_v21": "nnUNetPlansv2.1_plans_2D.pkl",
                                               "CustomExperimentPlanner": "custom_experiment_planner_plans_2D.pkl"}[planner]
    # use_nonzero_mask_for_norm went back into the cropped cases' .pkl files
    from cineflow.safe_pickle import load_plain_pickle
    for c in fx["cases"]:
        assert_same(load_plain_pickle(os.path.join(cropped, c + ".pkl")), fx["case_pkl"], c)


def test_branches_the_fixtures_are_there_for(planner_only):
    assert planner_only["lowres"]["plans"]["ExperimentPlanner3D_v21"]["num_stages"] == 2
    assert planner_only["shrink2d"]["case_pkl"]["use_nonzero_mask_for_norm"][0] is True
    assert list(planner_only["custom"]["plans"]["CustomExperimentPlanner"]["plans_per_stage"][0]["patch_size"]) == [288, 288]


def test_custom_planner_patch_follows_the_task_folder_name(tmp_path, planner_only):
    from cineflow import experiment_planning as EP
    fx = planner_only["custom"]
    cropped, _ = _folders(tmp_path, "custom", fx)
    pre = str(tmp_path / "Task027_ACDC")
    os.makedirs(pre)
    p = EP.CustomExperimentPlanner(cropped, pre, fx["config"])
    p.plan_experiment()
    assert list(p.plans["plans_per_stage"][0]["patch_size"]) == [224, 224]
    with pytest.raises(ValueError):
        EP.CustomExperimentPlanner(cropped, pre)


def test_written_plans_feed_the_importers(tmp_path, planner_only):
    from cineflow.reference_models import plans_from_reference, plans_from_reference_3d
    fx = planner_only["lowres"]
    for planner in ("ExperimentPlanner", "ExperimentPlanner3D_v21"):
        _, plans, _ = _plan(tmp_path, "lowres", fx, planner)          # (read back through load_plain_pickle)
        for stage in (0, 1):
            t = plans_from_reference_3d(plans, stage)
            assert t["patch_size"] == [int(v) for v in plans["plans_per_stage"][stage]["patch_size"]] and t["seg_net"]["dim"] == 3
        assert plans_from_reference_3d(plans)["stage"] == 1
    _, plans, _ = _plan(tmp_path, "lowres", fx, "ExperimentPlanner2D_v21")
    t = plans_from_reference(plans)
    assert t["patch_size"] == [int(v) for v in plans["plans_per_stage"][0]["patch_size"]]
    assert t["seg_net"]["base_num_features"] == 32 and t["num_classes"] == 4


def test_unknown_planner_name_raises():
    from cineflow import experiment_planning as EP
    from cineflow import plan_and_preprocess as PP
    assert EP.find_planner("None") is None and EP.find_planner(None) is None
    with pytest.raises(NotImplementedError, match="ExperimentPlanner3D_v21_Pretrained"):
        EP.find_planner("ExperimentPlanner3D_v21_Pretrained")
    with pytest.raises(NotImplementedError, match="ExperimentPlanner3DFabiansResUNet_v21"):      # before any file is touched
        PP.plan_and_preprocess("/nonexistent/raw", "/nonexistent/cropped", "/nonexistent/pre", planner3d="ExperimentPlanner3DFabiansResUNet_v21")


def test_vram_estimate_and_pool_props_on_known_values():
    """generic_UNet.py's own reference points: the 3-D constant is the estimate of its default 128^3-class patch family"""
    from cineflow import experiment_planning as EP
    numpool, pools, convs, patch, div = EP.get_pool_and_conv_props([1.0, 1.0, 1.0], [128, 128, 128], 4, 999)
    assert numpool == [5, 5, 5] and pools == [[2, 2, 2]] * 5 and convs == [[3, 3, 3]] * 6 and list(patch) == [128, 128, 128] and list(div) == [32] * 3
    numpool, pools, convs, patch, div = EP.get_pool_and_conv_props_poolLateV2([24, 504, 512], 4, 999, [5.9999094, 0.50781202, 0.50781202])
    assert [int(v) for v in numpool] == [2, 6, 7] and pools[0] == [1, 1, 2] and pools[-1] == [2, 2, 2] and list(patch) == [24, 512, 512]
    assert list(EP.pad_shape([10, 33, 64], [4, 32, 32])) == [12, 64, 64]
    v = EP.Generic_UNet.compute_approx_vram_consumption([64, 64], [2, 2], 8, 32, 1, 2, [[2, 2], [2, 2]])
    # 5 * 4096 * 8 + 4096 + 2 * 4096  +  5 * 1024 * 16  +  2 * 256 * 32
    assert v == 163840 + 12288 + 81920 + 16384 and isinstance(v, np.int64)


def test_select_entries_refuse_bad_arguments_without_a_gpu():
    from cineflow import _lib
    h = _lib.lib()
    vals = (ctypes.c_float * 17)(*range(17))
    vp = ctypes.cast(vals, ctypes.c_void_p)
    assert h.cf_select_blocks(1005) == 4 and h.cf_select_blocks(0) == 0
    # cf_select_count(key, n, values, n_values, mode, prefix, totals, stream); made-up addresses are never dereferenced
    assert h.cf_select_count(1, 1 << 31, vp, 2, 0, 1, 1, None) == -1 and b"2^31" in h.cf_last_error()
    assert h.cf_select_count(1, 100, vp, 17, 0, 1, 1, None) == -1 and b"1..16 values" in h.cf_last_error()
    assert h.cf_select_count(1, 100, vp, 0, 0, 1, 1, None) == -1
    for args in ((None, 100, vp, 2, 0, 1, 1), (1, 100, None, 2, 0, 1, 1), (1, 100, vp, 2, 0, None, 1), (1, 100, vp, 2, 0, 1, None), (None, 100, None, 0, 1, 1, 1)):
        assert h.cf_select_count(*args, None) == -1 and b"null pointer" in h.cf_last_error(), args
    assert h.cf_select_count(1, 100, vp, 2, 2, 1, 1, None) == -1 and b"mode" in h.cf_last_error()
    # cf_select_rank(key, n, mode, value, prefix, ranks, K, src, vals, coords, D0, D1, D2, stream)
    assert h.cf_select_rank(1, 1 << 31, 0, 1.0, 1, 1, 4, None, None, 1, 1, 1, 1, None) == -1 and b"2^31" in h.cf_last_error()
    assert h.cf_select_rank(1, 100, 0, 1.0, 1, 1, -1, None, None, 1, 4, 5, 5, None) == -1 and b"negative" in h.cf_last_error()
    for args in ((None, 100, 0, 1.0, 1, 1, 4, None, None, 1, 4, 5, 5), (1, 100, 0, 1.0, None, 1, 4, None, None, 1, 4, 5, 5),
                 (1, 100, 0, 1.0, 1, None, 4, None, None, 1, 4, 5, 5), (1, 100, 1, 0.0, 1, 1, 4, 1, None, None, 0, 0, 0)):
        assert h.cf_select_rank(*args, None) == -1 and b"null pointer" in h.cf_last_error(), args
    assert h.cf_select_rank(1, 100, 0, 1.0, 1, 1, 4, None, None, None, 4, 5, 5, None) == -1          # neither src nor coords
    assert h.cf_select_rank(1, 100, 0, 1.0, 1, 1, 4, 1, 1, 1, 4, 5, 5, None) == -1                   # both
    assert h.cf_select_rank(1, 100, 0, 1.0, 1, 1, 4, None, None, 1, 4, 5, 6, None) == -1 and b"does not hold" in h.cf_last_error()
    # K == 0 is valid and launches nothing
    assert h.cf_select_rank(1, 100, 0, 1.0, 1, None, 0, None, None, 1, 4, 5, 5, None) == 0


def test_select_wrappers_reject_cpu_tensors():
    import torch
    from cineflow import ops
    for call in (lambda: ops.label_counts(torch.zeros(2, 3, 4), [1]), lambda: ops.select_coords(torch.zeros(2, 3, 4), 1, [0]),
                 lambda: ops.select_values(torch.zeros(24), torch.zeros(24), [0])):
        with pytest.raises(TypeError):
            call()
