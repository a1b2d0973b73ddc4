"""python -m cineflow.model_selection on the device against tests/golden/model_selection: what the reference's consolidate_folds, its
model_selection ensemble() and the choice part of figure_out_what_to_submit.main made of the same seeded trees
(make_golden_model_selection.py; tree A: an ensemble wins, tree B: a single model wins, one fp32 model, two regions .pkl).

Label files are compared voxel for voxel; every summary.json the way tests/test_gpu_determine_postprocessing.py compares the evaluator's
output with its golden (every confusion-type value of 'all' and 'mean' with ==, NaN matching NaN, the same keys everywhere; the surface
metrics are "parity unpinned" in the fixture and are not compared); decisions, the chosen model, prediction_commands.txt and summary.csv
with ==.  Each tree is run once, in this process, through the module's main() with every native entry point counted, and shared by the
tests that read it; one test starts the command line itself."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "model_selection")
SURFACE = ("Hausdorff Distance", "Hausdorff Distance 95", "Avg. Symmetric Surface Distance")


def generator():
    spec = importlib.util.spec_from_file_location("make_golden_model_selection", os.path.join(HERE, "golden", "make_golden_model_selection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden(tag):
    with open(os.path.join(GOLDEN, tag + ".json")) as f:
        return dict(np.load(os.path.join(GOLDEN, tag + ".npz"))), json.load(f)


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def assert_results_equal(got, want, where):
    """`results` of a summary.json: every confusion-type value of 'all' and 'mean' with ==; the same keys everywhere"""
    assert len(got["all"]) == len(want["all"]), where
    for g, w in list(zip(got["all"], want["all"])) + [(got["mean"], want["mean"])]:
        assert set(g) == set(w), (where, set(g) ^ set(w))
        for label in w:
            if label in ("test", "reference"):
                assert os.path.basename(g[label]) == os.path.basename(w[label]), where
                continue
            assert set(g[label]) == set(w[label]), (where, label)
            for metric, value in w[label].items():
                if metric not in SURFACE:
                    assert same(g[label][metric], value), (where, label, metric, g[label][metric], value)


class CountingLib:
    """the native library with every cf_ call appended to `events`"""

    def __init__(self, real, events):
        self.real, self.events = real, events

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("cf_") or name == "cf_last_error":
            return fn

        def counted(*args):
            self.events.append(name)
            return fn(*args)
        return counted


def spied_main(argv):
    """cineflow.model_selection.main(argv) -> (its return value, events): every native call by name, and "<" / ">" around each
    determine_postprocessing / consolidate_folds (what lies outside them is the pair scoring)"""
    from cineflow import _lib, evaluation, metrics, model_selection as MS, ops, postprocessing
    events = []
    counter = CountingLib(_lib.lib(), events)
    mp = pytest.MonkeyPatch()
    try:
        for mod in (ops, evaluation, metrics, postprocessing):
            if hasattr(mod, "lib"):
                mp.setattr(mod, "lib", lambda: counter)

        def bracket(fn):
            def inner(*a, **k):
                events.append("<")
                try:
                    return fn(*a, **k)
                finally:
                    events.append(">")
            return inner
        mp.setattr(MS, "determine_postprocessing", bracket(MS.determine_postprocessing))
        mp.setattr(MS, "consolidate_folds", bracket(MS.consolidate_folds))
        best = MS.main(argv)
    finally:
        mp.undo()
    return best, events


def outside(events):
    depth, out = 0, []
    for e in events:
        if e == "<":
            depth += 1
        elif e == ">":
            depth -= 1
        elif depth == 0:
            out.append(e)
    return out


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """tag -> (G, fx, golden json, models [(NAME, folder)], root, out, best, events), one run per tree"""
    done = {}

    def run(tag):
        if tag not in done:
            G = generator()
            fx, js = golden(tag)
            root = str(tmp_path_factory.mktemp("ms_" + tag))
            models = G.build_tree(os.path.join(root, "trained"), fx)
            out = os.path.join(root, "out")
            argv = ["-m"] + ["%s=%s" % nf for nf in models] + ["-gt", os.path.join(root, "trained", "gt"), "-o", out, "-f", "0", "1", "-t", G.TASK]
            best, events = spied_main(argv)
            done[tag] = (G, fx, js, models, root, out, best, events, argv)
        return done[tag]
    return run


def pair_base(out, G, name):
    return os.path.join(out, "ensembles", G.TASK, name)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_label_files_equal_the_reference(runs, tag):
    from cineflow.nifti import read_nifti
    G, fx, js, _, _, out, _, _, _ = runs(tag)
    assert sorted(os.listdir(os.path.join(out, "ensembles", G.TASK))) == sorted(js["pairs"])
    for name in js["pairs"]:
        for folder in ("ensembled_raw", "ensembled_postprocessed"):
            for case in (str(c) for c in fx["cases"]):
                got = read_nifti(os.path.join(pair_base(out, G, name), folder, case + ".nii.gz"))[0]
                want = fx["%s/%s/%s" % (folder, name, case)]
                assert got.shape == want.shape and np.array_equal(got, want), "%s %s %s: %d voxels differ" % (name, folder, case, int((got != want).sum()))
    if tag == "A":                                          # the files are not trivially alike: the pairs differ, and postprocessing changed something
        first, second = list(js["pairs"])[:2]
        assert any((fx["ensembled_raw/%s/%s" % (first, c)] != fx["ensembled_raw/%s/%s" % (second, c)]).any() for c in fx["cases"])
        assert any((fx["ensembled_raw/%s/%s" % (first, c)] != fx["ensembled_postprocessed/%s/%s" % (first, c)]).any() for c in fx["cases"])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_summaries_equal_the_reference(runs, tag):
    G, fx, js, _, _, out, _, _, _ = runs(tag)
    for name, want in js["pairs"].items():
        base = pair_base(out, G, name)
        with open(os.path.join(base, "ensembled_raw", "summary.json")) as f:
            raw = json.load(f)
        assert raw["name"] == want["summary_raw_name"] and raw["task"] == G.TASK and raw["author"] == "Fabian"
        added = raw["results"]["mean"].pop("mean")                               # foreground_mean's entry, added after the reference's file was recorded
        assert added["Dice"] == float(np.nanmean([raw["results"]["mean"][str(c)]["Dice"] for c in G.CLASSES]))
        assert_results_equal(raw["results"], want["summary_raw"], "%s %s raw" % (tag, name))
        with open(os.path.join(base, "ensembled_postprocessed", "summary.json")) as f:
            final = json.load(f)
        assert final["experiment_name"] == name
        assert_results_equal(final["results"], want["summary_postprocessed"], "%s %s postprocessed" % (tag, name))
        with open(os.path.join(out, "summary_jsons", "%s__%s.json" % (G.TASK, name))) as f:
            assert json.dumps(json.load(f), sort_keys=True) == json.dumps(final, sort_keys=True)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_postprocessing_decisions_equal_the_reference(runs, tag):
    G, fx, js, _, _, out, _, _, _ = runs(tag)
    for name, entry in js["pairs"].items():
        want = entry["postprocessing"]
        with open(os.path.join(pair_base(out, G, name), "postprocessing.json")) as f:
            got = json.load(f)
        assert set(got) == set(want)
        for key in ("for_which_classes", "min_valid_object_sizes", "num_samples", "validation_raw", "validation_final"):
            assert got[key] == want[key], (name, key, got[key], want[key])
        for key in ("dc_per_class_raw", "dc_per_class_pp_all", "dc_per_class_pp_per_class"):
            assert set(got[key]) == set(want[key]), (name, key)
            for c, v in want[key].items():
                assert same(got[key][c], v), (name, key, c, got[key][c], v)
        assert got["validation_raw"] == "ensembled_raw" and got["validation_final"] == "ensembled_postprocessed"


@pytest.mark.parametrize("tag", ["A", "B"])
def test_the_choice_and_its_texts_equal_the_reference(runs, tag):
    G, fx, js, models, _, out, best, _, _ = runs(tag)
    assert best == (js["best"] if js["best"].startswith("ensemble") else G.model_name(js["best"]))
    assert best.startswith("ensemble") == (tag == "A")
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read() == G.expected_commands(js["commands"], dict(models), out)
    with open(os.path.join(out, "summary.csv")) as f:
        assert f.read() == G.expected_csv(js["csv"])


@pytest.mark.parametrize("tag", ["A", "B"])
def test_one_launch_per_case_scores_every_pair(runs, tag):
    G, fx, js, _, _, _, _, events, _ = runs(tag)
    scoring = outside(events)
    assert scoring.count("cf_ensemble_pairs") == len(fx["cases"]), scoring
    assert "cf_ensemble_merge" not in scoring and "cf_label_confusion" not in scoring and "cf_confusion_counts" not in scoring, scoring
    assert set(scoring) == {"cf_ensemble_pairs"}, sorted(set(scoring))
    assert events.count("<") == len(fx["models"]) + len(js["pairs"])              # consolidate_folds per model, determine_postprocessing per pair


def test_a_second_run_launches_nothing(runs):
    G, fx, js, models, _, out, best, _, argv = runs("B")
    before = {name: os.path.getmtime(os.path.join(pair_base(out, G, name), "ensembled_raw", str(fx["cases"][0]) + ".nii.gz")) for name in js["pairs"]}
    again, events = spied_main(argv)
    assert again == best
    assert [e for e in events if e not in "<>"] == [] and events == []             # nothing native, no postprocessing either
    for name, t in before.items():
        assert os.path.getmtime(os.path.join(pair_base(out, G, name), "ensembled_raw", str(fx["cases"][0]) + ".nii.gz")) == t
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read() == G.expected_commands(js["commands"], dict(models), out)


def test_a_missing_file_is_made_again_and_scored_from_the_files(runs):
    """skip rules: with one label file and one summary.json removed, only that case is visited again, and the summary is built from the
    label files of the cases that were not visited (they bring no counts) -- to the same document"""
    G, fx, js, models, _, out, best, _, argv = runs("B")
    name = list(js["pairs"])[0]
    folder = os.path.join(pair_base(out, G, name), "ensembled_raw")
    case = str(fx["cases"][1])
    os.remove(os.path.join(folder, case + ".nii.gz"))
    os.remove(os.path.join(folder, "summary.json"))
    _, events = spied_main(argv)
    assert events.count("cf_ensemble_pairs") == 1 and events.count("cf_label_confusion") == len(fx["cases"]) - 1 and "<" not in events
    from cineflow.nifti import read_nifti
    assert np.array_equal(read_nifti(os.path.join(folder, case + ".nii.gz"))[0], fx["ensembled_raw/%s/%s" % (name, case)])
    with open(os.path.join(folder, "summary.json")) as f:
        raw = json.load(f)["results"]
    raw["mean"].pop("mean")
    assert_results_equal(raw, js["pairs"][name]["summary_raw"], name)


def test_regions_class_order_from_pkl_changes_the_two_region_cases(runs, tmp_path):
    """--regions_class_order_from_pkl: the cases whose .pkl records an order are labelled by the region rule, the others as before"""
    from cineflow import model_selection as MS
    from cineflow.nifti import read_nifti
    G, fx, js, models, root, _, _, _, _ = runs("B")
    base = str(tmp_path / "ensembles" / G.TASK / MS.ensemble_name(models[0][0], models[2][0]))
    MS.ensemble(models[0][1], models[2][1], base, G.TASK, "validation_raw", G.FOLDS, os.path.join(root, "trained", "gt"), allow_ensembling=False,
                regions_class_order_from_pkl=True)
    name = os.path.basename(base)
    regions = [int(v) for v in fx["regions"]]
    for i, case in enumerate(str(c) for c in fx["cases"]):
        got = read_nifti(os.path.join(base, "ensembled_raw", case + ".nii.gz"))[0]
        a, b = fx["softmax/2d/" + case], fx["softmax/3d_lowres/" + case]
        if i in regions:
            mean = np.mean((a, b), 0)
            seg = np.zeros(mean.shape[1:], np.uint8)
            for k, c in enumerate(G.REGIONS_ORDER):
                seg[mean[k] > 0.5] = c
            lo = [int(v) for v in fx["lo/" + case]]
            want = np.zeros(fx["gt/" + case].shape, np.uint8)
            want[lo[0]:lo[0] + seg.shape[0], lo[1]:lo[1] + seg.shape[1], lo[2]:lo[2] + seg.shape[2]] = seg
        else:
            want = fx["ensembled_raw/%s/%s" % (name, case)]
        assert np.array_equal(got, want), case
    assert not os.path.exists(os.path.join(base, "postprocessing.json"))


def test_the_command_line(runs, tmp_path):
    """python -m cineflow.model_selection --disable_postprocessing on tree B, in a process of its own: the single model wins there too, the
    pairs' rows of summary.csv are the reference's (a single model's row comes from evaluate_folder here, which scores label 1 under the
    fork's rv_rejection, so it is not compared), and no postprocessing file is written"""
    G, fx, js, models, root, _, _, _, _ = runs("B")
    fresh = G.build_tree(str(tmp_path / "trained"), fx)
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(os.path.dirname(HERE), "cardiac-segmentation-optical-flow_amd")]
                                                      + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    done = subprocess.run([sys.executable, "-m", "cineflow.model_selection", "-m"] + ["%s=%s" % nf for nf in fresh]
                          + ["-gt", str(tmp_path / "trained" / "gt"), "-o", out, "-f", "0", "1", "-t", G.TASK, "--disable_postprocessing"],
                          env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(os.path.join(out, "prediction_commands.txt")) as f:
        assert f.read() == G.expected_commands(js["commands"], dict(fresh), out)
    with open(os.path.join(out, "summary.csv")) as f:
        rows = f.read().splitlines()
    want = G.expected_csv(js["csv"]).splitlines()
    assert [r.split(",")[0] for r in rows] == [r.split(",")[0] for r in want]
    assert [r for r in rows if r.startswith("ensemble_")] == [r for r in want if r.startswith("ensemble_")] and len(rows) == 7
    assert not os.path.exists(os.path.join(fresh[0][1], "postprocessing.json"))
    assert not os.path.exists(os.path.join(pair_base(out, G, list(js["pairs"])[0]), "postprocessing.json"))
