"""cineflow.validate without a GPU: do_split against tests/golden/validate/splits.json (scikit-learn's KFold under the fork's pairing of
adjacent cases, make_golden_validate.py), an existing splits_final.pkl, the seeded 80:20 branch, fold 'all', the refusal of an odd number
of cases and of a model folder with a flow network, load_dataset, the separate-z flags, and the command line."""
import json
import os
import pickle

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_splits():
    with open(os.path.join(HERE, "golden", "validate", "splits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("n", [10, 12])
def test_do_split_creates_the_forks_five_folds(tmp_path, n):
    from cineflow import validate as V
    from cineflow.safe_pickle import load_plain_pickle
    fx = golden_splits()[str(n)]
    splits_file = str(tmp_path / "splits_final.pkl")
    for fold, want in enumerate(fx["splits"]):
        tr, val = V.do_split(fx["keys"], fold, splits_file)
        assert tr == want["train"] and val == want["val"], fold
        assert sorted(tr + val) == sorted(fx["keys"])
    written = load_plain_pickle(splits_file)                       # what a later run (and the reference) reads back
    assert len(written) == 5
    for got, want in zip(written, fx["splits"]):
        assert [str(k) for k in got["train"]] == want["train"] and [str(k) for k in got["val"]] == want["val"]
    assert all(len(s["val"]) % 2 == 0 for s in fx["splits"])       # pairs stay together


@pytest.mark.parametrize("n", [5, 6, 11, 24])
def test_kfold_indices_equal_scikit_learn_where_it_is_installed(n):
    model_selection = pytest.importorskip("sklearn.model_selection")
    from cineflow import validate as V
    want = list(model_selection.KFold(n_splits=5, shuffle=True, random_state=12345).split(np.arange(n)))
    got = V.kfold_indices(n)
    assert len(got) == 5
    for (tr, te), (wtr, wte) in zip(got, want):
        assert np.array_equal(tr, wtr) and np.array_equal(te, wte)


def test_too_few_pairs_for_five_folds_are_refused(tmp_path):
    from cineflow import validate as V
    with pytest.raises(ValueError, match="n_splits=5"):
        V.do_split(["a", "b", "c", "d", "e", "f"], 0, str(tmp_path / "s.pkl"))
    assert not os.path.exists(str(tmp_path / "s.pkl"))


def test_an_existing_split_file_is_used(tmp_path):
    from cineflow import validate as V
    keys = ["c%d" % i for i in range(6)]
    splits = [{"train": np.array(["c0", "c1", "c5", "c4"]), "val": np.array(["c3", "c2"])}, {"train": np.array(["c2", "c3"]), "val": np.array(keys[:2] + keys[4:])}]
    splits_file = str(tmp_path / "splits_final.pkl")
    with open(splits_file, "wb") as f:
        pickle.dump(splits, f)
    before = open(splits_file, "rb").read()
    assert V.do_split(keys, 0, splits_file) == (["c0", "c1", "c4", "c5"], ["c2", "c3"])
    assert V.do_split(keys, 1, splits_file) == (["c2", "c3"], ["c0", "c1", "c4", "c5"])
    assert open(splits_file, "rb").read() == before
    with pytest.raises(KeyError, match="c3"):
        V.do_split(keys[:3], 0, splits_file)


def test_a_fold_beyond_the_file_gives_the_seeded_80_20_split(tmp_path):
    from cineflow import validate as V
    keys = ["case_%02d" % i for i in range(10)][::-1]
    splits_file = str(tmp_path / "splits_final.pkl")
    with open(splits_file, "wb") as f:
        pickle.dump([{"train": np.array(keys[:8]), "val": np.array(keys[8:])}], f)
    fold = 3
    tr, val = V.do_split(keys, fold, splits_file)
    ordered = sorted(keys)                                          # nnUNetTrainerV2.py:336-342
    idx = np.random.RandomState(seed=12345 + fold).choice(10, 8, replace=False)
    assert tr == sorted(ordered[i] for i in idx) and val == sorted(k for i, k in enumerate(ordered) if i not in idx)
    assert len(tr) == 8 and len(val) == 2 and sorted(tr + val) == ordered


def test_fold_all_takes_every_key_and_needs_no_file(tmp_path):
    from cineflow import validate as V
    splits_file = str(tmp_path / "splits_final.pkl")
    tr, val = V.do_split(["b", "c", "a"], "all", splits_file)
    assert tr == val == ["a", "b", "c"] and not os.path.exists(splits_file)


def test_an_odd_number_of_cases_is_refused(tmp_path):
    from cineflow import validate as V
    with pytest.raises(ValueError, match="11 cases.*even"):
        V.do_split(["k%02d" % i for i in range(11)], 0, str(tmp_path / "splits_final.pkl"))
    assert not os.path.exists(str(tmp_path / "splits_final.pkl"))


def test_load_dataset_lists_the_cases_of_a_stage_folder(tmp_path):
    from cineflow import validate as V
    for name in ("b.npz", "b.pkl", "a.npz", "a.pkl", "a_segFromPrevStage.npz", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    ds = V.load_dataset(str(tmp_path))
    assert list(ds) == ["a", "b"]
    assert ds["a"]["data_file"] == str(tmp_path / "a.npz") and ds["b"]["properties_file"] == str(tmp_path / "b.pkl")
    with pytest.raises(FileNotFoundError):
        V.load_dataset(str(tmp_path / "absent"))


def test_a_model_folder_with_a_flow_network_is_refused(tmp_path):
    from cineflow import validate as V
    from cineflow.trainer import default_plans
    model = tmp_path / "model"
    model.mkdir()
    (model / "plans.json").write_text(json.dumps(default_plans(image_size=64)))
    with pytest.raises(ValueError, match="flow_net"):
        V.check_model_folder(str(model))
    with pytest.raises(ValueError, match="flow_net"):                                # the command refuses before it loads anything
        V.main(["-m", str(model), "--data", str(tmp_path / "stage"), "-gt", str(tmp_path / "gt"), "-o", str(tmp_path / "out"), "-f", "0"])
    assert not (tmp_path / "out").exists()
    (model / "plans.json").write_text(json.dumps(default_plans(image_size=64, flow_variant=None)))
    assert "flow_net" not in V.check_model_folder(str(model))
    with pytest.raises(FileNotFoundError):
        V.check_model_folder(str(tmp_path / "nothing"))


def test_separate_z_flags_follow_the_exporters_decision():
    from cineflow import validate as V
    aniso = {"original_spacing": np.array([8.0, 1.4, 1.4]), "spacing_after_resampling": np.array([7.0, 1.4, 1.4])}
    iso = {"original_spacing": np.array([1.0, 1.0, 1.0]), "spacing_after_resampling": np.array([1.0, 1.0, 1.0])}
    after = {"original_spacing": np.array([1.0, 1.0, 1.0]), "spacing_after_resampling": np.array([1.0, 1.0, 5.0])}
    two = {"original_spacing": np.array([8.0, 8.0, 1.0]), "spacing_after_resampling": np.array([8.0, 8.0, 1.0])}
    assert V.linear_flags(aniso, None, 1, 0) == (0, 1, 1)
    assert V.linear_flags(aniso, None, 1, 1) == (1, 1, 1)
    assert V.linear_flags(aniso, False, 1, 0) == (1, 1, 1)
    assert V.linear_flags(iso, None, 1, 0) == (1, 1, 1)
    assert V.linear_flags(iso, None, 0, 0) == (0, 0, 0)
    assert V.linear_flags(after, None, 1, 0) == (1, 1, 0)
    assert V.linear_flags(two, None, 1, 0) == (1, 1, 1)                # two low-resolution axes: not separate
    assert V.linear_flags(after, True, 1, 0) == (1, 1, 1)              # forced: the axis comes from original_spacing, which names three
    with pytest.raises(NotImplementedError):
        V.linear_flags(iso, None, 3, 0)


def test_command_line_parsing(tmp_path):
    from cineflow import validate as V
    a = V.build_parser().parse_args(["-m", "M", "--data", "D", "-gt", "G", "-o", "O"])
    assert (a.model_folder, a.data, a.gt_folder, a.output_folder) == ("M", "D", "G", "O")
    assert a.folds is None and a.splits is None and a.plans is None and a.val == "validation_raw" and a.step_size == 0.5 and a.overwrite == 1
    assert not (a.no_softmax or a.disable_tta or a.disable_postprocessing or a.debug) and a.next_stage is None and a.prev_stage is None
    a = V.build_parser().parse_args(["-m", "M", "--data", "D", "-gt", "G", "-o", "O", "-f", "0", "3", "all", "--splits", "S", "--plans", "P", "--val", "v",
                                     "--no_softmax", "--disable_tta", "--step_size", "0.75", "--overwrite", "0", "--disable_postprocessing", "--debug",
                                     "--next_stage", "N", "--prev_stage", "L", "-t", "Task501"])
    assert a.folds == ["0", "3", "all"] and (a.splits, a.plans, a.val, a.next_stage, a.prev_stage, a.task) == ("S", "P", "v", "N", "L", "Task501")
    assert a.no_softmax and a.disable_tta and a.disable_postprocessing and a.debug and a.step_size == 0.75 and a.overwrite == 0
    assert V.parse_folds(a.folds, "unused") == [0, 3, "all"]
    for d in ("fold_1", "fold_0", "all"):
        (tmp_path / d).mkdir()
    assert V.parse_folds(None, str(tmp_path)) == [0, 1]
    with pytest.raises(SystemExit):
        V.build_parser().parse_args(["-m", "M"])
