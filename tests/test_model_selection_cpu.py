"""cineflow.model_selection without a GPU: the folder checks of `ensemble` and their messages, pair naming and order, get_foreground_mean and
the exact-tie rule of the choice, summary.csv and prediction_commands.txt against tests/golden/model_selection (the reference's own text;
make_golden_model_selection.py's expected_commands / expected_csv state the two deliberate differences: this project's commands, and a
single model named by its full NAME), and the host-side argument validation of cf_ensemble_pairs, which launches nothing when it refuses."""
import ctypes
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "model_selection")


def generator():
    spec = importlib.util.spec_from_file_location("make_golden_model_selection", os.path.join(HERE, "golden", "make_golden_model_selection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden(tag):
    with open(os.path.join(GOLDEN, tag + ".json")) as f:
        return dict(np.load(os.path.join(GOLDEN, tag + ".npz"))), json.load(f)


@pytest.fixture()
def tree(tmp_path):
    G = generator()
    fx, _ = golden("B")
    return G, G.build_tree(str(tmp_path / "trained"), fx), str(tmp_path)


# ------------------------------------------------------------------------------------------------ ensemble(): the folder checks
def _ensemble(named, root, G):
    from cineflow import model_selection as MS
    MS.ensemble(named[0][1], named[1][1], os.path.join(root, "out", "ensembles", G.TASK, MS.ensemble_name(named[0][0], named[1][0])), G.TASK,
                "validation_raw", G.FOLDS, os.path.join(root, "trained", "gt"))


def _val(named, n, fold):
    return os.path.join(named[n][1], "fold_%d" % fold, "validation_raw")


@pytest.mark.parametrize("n,message", [(0, "Validation directory missing: %s. Please rerun validation with `nnUNet_train CONFIG TRAINER TASK FOLD -val --npz`"),
                                       (1, "Validation directory missing: %s. Please rerun validation with `nnUNet_train CONFIG TRAINER TASK FOLD -val --npz`")])
def test_a_missing_validation_directory(tree, n, message):
    G, named, root = tree
    shutil.rmtree(_val(named, n, 1))
    with pytest.raises(AssertionError) as e:
        _ensemble(named, root, G)
    assert str(e.value) == message % _val(named, n, 1)


@pytest.mark.parametrize("n,word", [(0, "incomplete"), (1, "missing")])
def test_a_missing_summary_json(tree, n, word):
    G, named, root = tree
    os.remove(os.path.join(_val(named, n, 0), "summary.json"))
    with pytest.raises(AssertionError) as e:
        _ensemble(named, root, G)
    assert str(e.value) == "Validation directory %s: %s. Please rerun validation with `nnUNet_train CONFIG TRAINER TASK FOLD -val --npz`" % (
        word, _val(named, n, 0))


@pytest.mark.parametrize("n", [0, 1])
def test_a_nii_without_its_npz(tree, n):
    G, named, root = tree
    os.remove(os.path.join(_val(named, n, 1), "case_02.npz"))
    with pytest.raises(AssertionError) as e:
        _ensemble(named, root, G)
    assert str(e.value) == "Missing npz files in folder %s. Please run the validation for all models and folds with the '--npz' flag." % _val(named, n, 1)


@pytest.mark.parametrize("rename", [False, True])
def test_identifier_lists_that_differ(tree, rename):
    G, named, root = tree
    for ext in (".npz", ".nii.gz", ".pkl"):
        src = os.path.join(_val(named, 1, 0), "case_01" + ext)
        if rename:
            os.rename(src, os.path.join(_val(named, 1, 0), "case_91" + ext))
        else:
            os.remove(src)
    with pytest.raises(AssertionError, match="npz filenames do not match. This should not happen."):
        _ensemble(named, root, G)


def test_postprocessed_and_noPostProcess_files_need_no_npz(tree, monkeypatch):
    """ensemble.py:77-78: such label files are not cases; the checks pass and the first case is visited"""
    from cineflow import model_selection as MS
    G, named, root = tree
    for name in ("case_00_postprocessed.nii.gz", "case_00_noPostProcess.nii.gz"):
        shutil.copy(os.path.join(_val(named, 0, 0), "case_00.nii.gz"), os.path.join(_val(named, 0, 0), name))

    class Reached(Exception):
        pass

    def visit(folders, wanted, fold, case, *a):
        assert (fold, case, wanted) == (0, "case_00", [(0, 1)])
        raise Reached()
    monkeypatch.setattr(MS, "_visit_case", visit)
    with pytest.raises(Reached):
        _ensemble(named, root, G)


# ------------------------------------------------------------------------------------------------ the choice
def test_get_foreground_mean_skips_background_and_mean():
    from cineflow import model_selection as MS
    doc = {"results": {"mean": {"0": {"Dice": 0.99}, "1": {"Dice": 0.5}, "2": {"Dice": 0.75}, "mean": {"Dice": 0.1}}}}
    assert MS.get_foreground_mean(doc) == np.mean([0.5, 0.75])
    doc["results"]["mean"]["3"] = {"Dice": float("nan")}
    assert np.isnan(MS.get_foreground_mean(doc))                                       # np.mean, not nanmean, as in the reference


def test_foreground_mean_adds_the_mean_entry(tmp_path):
    from cineflow import model_selection as MS
    path = str(tmp_path / "summary.json")
    with open(path, "w") as f:
        json.dump({"results": {"all": [], "mean": {"0": {"Dice": 1.0, "Jaccard": 1.0}, "1": {"Dice": 0.5, "Jaccard": 0.25},
                                                   "2": {"Dice": float("nan"), "Jaccard": 0.75}, "99": {"Dice": 0.0, "Jaccard": 0.0}}}}, f)
    MS.foreground_mean(path)
    with open(path) as f:
        mean = json.load(f)["results"]["mean"]
    assert "99" not in mean and mean["mean"] == {"Dice": 0.5, "Jaccard": 0.5}


def fabricate(tmp_path, monkeypatch, single, pairs):
    """model folders that need no device work (cv_niftis_raw/summary.json and postprocessing.json are there) and an _ensemble_pairs that
    writes the given pair summaries -> (models, out, the pair order it was asked for)"""
    from cineflow import model_selection as MS
    models = []
    for name, mean in single.items():
        folder = tmp_path / name
        (folder / "cv_niftis_raw").mkdir(parents=True)
        (folder / "postprocessing.json").write_text("{}")
        with open(str(folder / "cv_niftis_raw" / "summary.json"), "w") as f:
            json.dump({"results": {"all": [], "mean": mean}}, f)
        models.append((name, str(folder)))
    asked = []

    def fake(folders, wanted, bases, task, validation_folder, folds, gt_folder, allow_ensembling, regions, out_dir_all_json):
        for ab in wanted:
            name = os.path.basename(bases[ab])
            asked.append((ab, name, folders[ab[0]], folders[ab[1]]))
            os.makedirs(os.path.join(bases[ab], "ensembled_raw"))
            with open(os.path.join(bases[ab], "ensembled_raw", "summary.json"), "w") as f:
                json.dump({"results": {"all": [], "mean": pairs[name]}}, f)
    monkeypatch.setattr(MS, "_ensemble_pairs", fake)
    return models, str(tmp_path / "out"), asked


def dice(*values):
    return {str(c + 1): {"Dice": v} for c, v in enumerate(values)}


def test_pair_names_and_order(tmp_path, monkeypatch):
    from cineflow import model_selection as MS
    names = ["2d__T__P", "3d_fullres__T__P", "3d_lowres__T__P", "3d_cascade_fullres__TC__P"]
    pairs = {MS.ensemble_name(a, b): dice(0.5, 0.5) for a in names for b in names}
    models, out, asked = fabricate(tmp_path, monkeypatch, {n: dice(0.25, 0.5) for n in names}, pairs)
    best, results = MS.find_best_configuration(models, "gt", out, folds=(0, 1), task="Task007_X")
    assert [a[0] for a in asked] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]                  # itertools.combinations of the -m order
    assert asked[4][1] == "ensemble_3d_fullres__T__P--3d_cascade_fullres__TC__P"
    assert asked[4][2:] == (models[1][1], models[3][1])
    assert list(results) == names + [a[1] for a in asked]
    assert os.path.isdir(os.path.join(out, "ensembles", "Task007_X", asked[0][1]))


def test_an_exact_tie_appends_every_winner_and_names_the_last(tmp_path, monkeypatch):
    from cineflow import model_selection as MS
    a, b = "2d__T__P", "3d_fullres__T__P"
    models, out, _ = fabricate(tmp_path, monkeypatch, {a: dice(0.75, 0.5), b: dice(0.5, 0.25)}, {MS.ensemble_name(a, b): dice(0.5, 0.75)})
    best, results = MS.find_best_configuration(models, "gt", out, task="T1")
    assert results[a] == results[MS.ensemble_name(a, b)] == 0.625 and best == MS.ensemble_name(a, b)
    pp = os.path.join(out, "ensembles", "T1", best, "postprocessing.json")
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read() == ("python -m cineflow.predict -i FOLDER_WITH_TEST_CASES -o OUTPUT_FOLDER_MODEL1 -m %s\n"
                            "python -m cineflow.predict -i FOLDER_WITH_TEST_CASES -o OUTPUT_FOLDER_MODEL1 -m %s -z\n"
                            "python -m cineflow.predict -i FOLDER_WITH_TEST_CASES -o OUTPUT_FOLDER_MODEL2 -m %s -z\n"
                            "python -m cineflow.ensemble_predictions -f OUTPUT_FOLDER_MODEL1 OUTPUT_FOLDER_MODEL2 -o OUTPUT_FOLDER -pp %s\n"
                            % (models[0][1], models[0][1], models[1][1], pp))


def test_disable_ensembling_and_postprocessing(tmp_path, monkeypatch):
    from cineflow import model_selection as MS
    a, b = "2d__T__P", "3d_fullres__T__P"
    models, out, asked = fabricate(tmp_path, monkeypatch, {a: dice(0.5), b: dice(0.75)}, {MS.ensemble_name(a, b): dice(0.875)})
    best, _ = MS.find_best_configuration(models, "gt", out, disable_ensembling=True, disable_postprocessing=True)
    assert best == b and asked == []
    best, _ = MS.find_best_configuration(models, "gt", out, disable_postprocessing=True)
    assert best == MS.ensemble_name(a, b)
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read().splitlines()[-1] == "python -m cineflow.ensemble_predictions -f OUTPUT_FOLDER_MODEL1 OUTPUT_FOLDER_MODEL2 -o OUTPUT_FOLDER"


@pytest.mark.parametrize("tag", ["A", "B"])
def test_csv_and_commands_equal_the_reference(tmp_path, monkeypatch, tag):
    """the reference's per-model and per-pair means in, its summary.csv and prediction_commands.txt out"""
    from cineflow import model_selection as MS
    G = generator()
    _, js = golden(tag)
    single = {G.model_name(m): {k: v for k, v in mean.items() if k != "mean"} for m, mean in js["single_mean"].items()}
    pairs = {name: p["summary_raw"]["mean"] for name, p in js["pairs"].items()}
    models, out, asked = fabricate(tmp_path, monkeypatch, single, pairs)
    best, results = MS.find_best_configuration(models, "gt", out, folds=G.FOLDS, task=G.TASK)
    assert best == (js["best"] if js["best"].startswith("ensemble") else G.model_name(js["best"]))
    assert [a[1] for a in asked] == list(js["pairs"]) or sorted(a[1] for a in asked) == sorted(js["pairs"])
    for name, value in js["results"].items():
        assert results[name if name.startswith("ensemble") else G.model_name(name)] == value
    with open(os.path.join(out, "summary.csv")) as f:
        assert f.read() == G.expected_csv(js["csv"])
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read() == G.expected_commands(js["commands"], dict(models), out)


def test_parse_models():
    from cineflow import model_selection as MS
    assert list(MS.parse_models(["2d__T__P=/a", "3d_fullres__T__P=/b=c"]).items()) == [("2d__T__P", "/a"), ("3d_fullres__T__P", "/b=c")]
    for bad in (["2d__T__P"], ["2d=/a"], ["2d__T__P=/a", "2d__T__P=/b"], ["a--b__T__P=/a"]):
        with pytest.raises(ValueError):
            MS.parse_models(bad)
    args = MS.build_parser().parse_args(["-m", "2d__T__P=/a", "-gt", "/g", "-o", "/o", "-f", "0", "1"])
    assert args.folds == [0, 1] and args.validation_folder == "validation_raw" and not args.disable_ensembling


# ------------------------------------------------------------------------------------------------ Evaluator: a ready histogram
def test_evaluator_from_a_ready_histogram_equals_the_per_label_matrices():
    from cineflow import evaluation as E
    rng = np.random.default_rng(5)
    test, ref = rng.integers(0, 4, size=(3, 7, 9)), rng.integers(0, 4, size=(3, 7, 9))
    hist = np.bincount((test * 16 + ref).ravel(), minlength=256).reshape(16, 16)
    got = E.Evaluator(labels=[1, 2, 3]).evaluate(histogram=(hist, test.size))
    for c in (1, 2, 3):
        tp, fp = int(((test == c) & (ref == c)).sum()), int(((test == c) & (ref != c)).sum())
        fn, tn = int(((test != c) & (ref == c)).sum()), int(((test != c) & (ref != c)).sum())
        want = {"Dice": 2.0 * tp / (2 * tp + fp + fn), "Jaccard": tp / (tp + fp + fn), "Precision": tp / (tp + fp), "Recall": tp / (tp + fn),
                "Accuracy": (tp + tn) / (tp + fp + tn + fn), "True Negative Rate": tn / (tn + fp),
                "Total Positives Test": tp + fp, "Total Positives Reference": tp + fn}
        for m, v in want.items():
            assert got[str(c)][m] == v, (c, m, got[str(c)][m], v)
        assert set(got[str(c)]) == set(E.Evaluator.default_metrics)
    with pytest.raises(ValueError, match="surface metrics need the volumes"):
        E.Evaluator(labels=[1]).evaluate(histogram=(hist, test.size), advanced=True)
    with pytest.raises(ValueError, match="not answered by the histogram"):
        E.Evaluator(labels=[16]).evaluate(histogram=(hist, test.size))
    res = E.aggregate_scores([(E.Counted("a.nii.gz", hist, test.size), "gt/a.nii.gz")], labels=[1, 2, 3])
    assert res["all"][0]["test"] == "a.nii.gz" and res["all"][0]["reference"] == "gt/a.nii.gz" and res["mean"]["2"] == dict(got["2"])


# ------------------------------------------------------------------------------------------------ cf_ensemble_pairs: host-side validation
def _call(h, n=3, dtype=0, K=4, crop=(5, 13, 17), full=(7, 16, 24), lo=(1, 2, 3), pairs=((0, 1), (0, 2), (1, 2)), n_pairs=None, members=True, gt=1,
          seg=1, hist=1, null_member=None):
    ptrs = (ctypes.c_void_p * 9)(*([0x1000] * 9))                   # never dereferenced on the device: every call below is refused on the host
    if null_member is not None:
        ptrs[null_member] = None
    flat = (ctypes.c_int * 60)(*([v for ij in pairs for v in ij] + [0, 1] * (30 - len(pairs))))
    return h.cf_ensemble_pairs(ctypes.cast(ptrs, ctypes.c_void_p) if members else None, n, dtype, K, *crop, ctypes.cast(flat, ctypes.c_void_p),
                               len(pairs) if n_pairs is None else n_pairs, gt, seg, *full, *lo, None, hist, None)


@pytest.mark.parametrize("kwargs,text", [(dict(n=1), b"n_members = 1 is outside 2..8"),
                                         (dict(n=9), b"n_members = 9 is outside 2..8"),
                                         (dict(n_pairs=0), b"n_pairs = 0 is outside 1..28"),
                                         (dict(n_pairs=29), b"n_pairs = 29 is outside 1..28"),
                                         (dict(pairs=((0, 1), (1, 1))), b"pair 1 = (1, 1) names one member twice"),
                                         (dict(pairs=((0, 3),)), b"pair 0 = (0, 3) names a member outside 0..2"),
                                         (dict(pairs=((0, 1), (-1, 2))), b"pair 1 = (-1, 2) names a member outside 0..2"),
                                         (dict(lo=(1, 2, 8)), b"overhangs the volume"),           # 8 + 17 > 24
                                         (dict(lo=(3, 2, 3)), b"overhangs the volume"),
                                         (dict(lo=(1, -1, 3)), b"overhangs the volume"),
                                         (dict(null_member=2), b"member 2 is a null pointer"),
                                         (dict(members=False), b"null pointer"),
                                         (dict(gt=None), b"null pointer"),
                                         (dict(seg=None), b"null pointer"),
                                         (dict(hist=None), b"null pointer"),
                                         (dict(dtype=2), b"dtype = 2"),
                                         (dict(K=0), b"K = 0 is outside 1..255"),
                                         (dict(crop=(5, 0, 17)), b"bad shape")])
def test_cf_ensemble_pairs_validates_on_the_host(kwargs, text):
    from cineflow import _lib
    h = _lib.lib()
    rc = _call(h, **kwargs)
    assert rc != 0 and b"cf_ensemble_pairs" in h.cf_last_error() and text in h.cf_last_error(), (rc, h.cf_last_error())
