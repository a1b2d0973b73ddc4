"""cineflow.evaluation / cineflow.postprocessing on the device against tests/golden/postprocessing: what the reference's aggregate_scores,
determine_postprocessing (plain and advanced) and consolidate_folds wrote for the same seeded folders (make_golden_postprocessing.py).

Decisions, thresholds, Dice tables and every confusion-type value of every summary.json are compared with == (the same integers through the
same float64 expressions; NaN matches NaN); final and temporary volumes voxel for voxel.  The surface metrics are "parity unpinned" in the
fixture (medpy is absent where it was made), so they are compared with cineflow.metrics called directly, with == as well.  Each folder is run once and shared
by the tests that read it."""
import json
import math
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocessing")
SPACING = (1.25, 1.25, 8.0)
CLASSES = [1, 2, 3]
SURFACE = ("Hausdorff Distance", "Hausdorff Distance 95", "Avg. Symmetric Surface Distance")


def fixture(tag):
    """(arrays, {"postprocessing": the reference's postprocessing.json, "summary_<folder>": its summary.json `results`, rebuilt from the arrays
    [cases + mean, classes, metrics] the generator packed them into})"""
    fx = dict(np.load(os.path.join(GOLDEN, tag + ".npz")))
    with open(os.path.join(GOLDEN, "decisions.json")) as f:
        js = {"postprocessing": json.load(f)[tag]}
    names = [str(m) for m in fx["summary_metrics"]]
    for key in ("raw", "final", "temp_allClasses", "temp_perClass"):
        if "summary_" + key in fx:
            rows = [{str(c + 1): dict(zip(names, (float(v) for v in per_class))) for c, per_class in enumerate(row)} for row in fx["summary_" + key]]
            for row, test in zip(rows, fx["summary_%s_tests" % key]):
                row["test"] = row["reference"] = str(test)
            js["summary_" + key] = {"all": rows[:-1], "mean": rows[-1]}
    return fx, js


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


def write_tree(base, fx):
    from cineflow.nifti import write_nifti
    names = [str(n) for n in fx["names"]]
    os.makedirs(os.path.join(base, "validation_raw"))
    os.makedirs(os.path.join(base, "gt"))
    for n, p, g in zip(names, fx["pred"], fx["gt"]):
        write_nifti(os.path.join(base, "validation_raw", n), p, SPACING)
        if "_u" not in n:
            write_nifti(os.path.join(base, "gt", n), g, SPACING)
    return names


def read_stack(folder, names):
    from cineflow.nifti import read_nifti
    return np.stack([read_nifti(os.path.join(folder, n))[0] for n in names])


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """tag -> (base folder, names, raw `results`): aggregate_scores then determine_postprocessing, once per folder"""
    from cineflow import evaluation as E
    from cineflow import postprocessing as PP
    done = {}

    def run(tag):
        if tag not in done:
            fx, _ = fixture(tag)
            base = str(tmp_path_factory.mktemp("pp_" + tag))
            names = write_tree(base, fx)
            pairs = [(os.path.join(base, "validation_raw", n), os.path.join(base, "gt", n)) for n in names if "_u" not in n]
            raw = E.aggregate_scores(pairs, labels=CLASSES, json_output_file=os.path.join(base, "validation_raw", "summary.json"), advanced=True,
                                     nb_threads=2)
            PP.determine_postprocessing(base, os.path.join(base, "gt"), advanced_postprocessing=tag == "D", log_function=lambda *a: None,
                                        nb_threads=2)
            done[tag] = (base, names, raw)
        return done[tag]
    return run


@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_raw_summary_equals_the_reference(runs, tag):
    base, names, raw = runs(tag)
    _, js = fixture(tag)
    assert_results_equal(json.loads(json.dumps(raw)), js["summary_raw"], tag + " raw")
    with open(os.path.join(base, "validation_raw", "summary.json")) as f:
        written = json.load(f)
    assert set(written) == {"name", "description", "timestamp", "task", "author", "results", "id"} and written["author"] == "Fabian"
    assert_results_equal(written["results"], js["summary_raw"], tag + " raw file")


@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_decisions_and_dice_tables_equal_the_reference(runs, tag):
    from cineflow.export import load_postprocessing
    base, names, _ = runs(tag)
    _, js = fixture(tag)
    want = js["postprocessing"]
    with open(os.path.join(base, "postprocessing.json")) as f:
        got = json.load(f)
    assert set(got) == set(want) - {"min_valid_object_sizes_as_written"}
    for key in ("for_which_classes", "min_valid_object_sizes", "num_samples", "validation_raw", "validation_final"):
        assert got[key] == want[key], (tag, key, got[key], want[key])
    for key in ("dc_per_class_raw", "dc_per_class_pp_all", "dc_per_class_pp_per_class"):
        assert set(got[key]) == set(want[key]), (tag, key)
        for c, v in want[key].items():
            assert same(got[key][c], v), (tag, key, c, got[key][c], v)
    fwc, sizes = load_postprocessing(os.path.join(base, "postprocessing.json"))
    assert fwc == want["for_which_classes"]
    if tag == "D":
        assert sizes == {(1, 2, 3): 3900.0, 2: 1500.0} and isinstance(list(sizes)[0], tuple)
    else:
        assert sizes is None


@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_volumes_and_summaries_of_every_folder_equal_the_reference(runs, tag):
    base, names, _ = runs(tag)
    fx, js = fixture(tag)
    for key, folder in (("final", "validation_final"), ("temp_allClasses", "temp_allClasses"), ("temp_perClass", "temp_perClass")):
        got = read_stack(os.path.join(base, folder), names)
        assert got.dtype == fx[key].dtype and np.array_equal(got, fx[key]), "%s %s: %d voxels differ" % (tag, key, int((got != fx[key]).sum()))
        with open(os.path.join(base, folder, "summary.json")) as f:
            assert_results_equal(json.load(f)["results"], js["summary_" + key], "%s %s" % (tag, key))
    assert (fx["final"] != fx["pred"]).any() or tag == "C"


def test_surface_metrics_are_those_of_cineflow_metrics(runs):
    from cineflow import metrics as M
    base, names, _ = runs("A")
    fx, _ = fixture("A")
    with open(os.path.join(base, "validation_final", "summary.json")) as f:
        res = json.load(f)["results"]
    spacing = np.array(SPACING)[::-1]
    funcs = dict(zip(SURFACE, (M.hausdorff_distance, M.hausdorff_distance_95, M.avg_surface_distance_symmetric)))
    evaluated = [i for i, n in enumerate(names) if "_u" not in n]
    checked = 0
    for entry, i in zip(res["all"], evaluated):
        assert os.path.basename(entry["test"]) == names[i]
        for c in CLASSES:
            for metric, fn in funcs.items():
                # (summary values are taken with reproducible=True: the mean distances are summed in sorted order, so ASSD is one value for
                # one pair of masks whatever order the device found the border voxels in)
                direct = fn(fx["final"][i] == c, fx["gt"][i] == c, voxel_spacing=spacing, reproducible=True)
                assert same(entry[str(c)][metric], direct), (names[i], c, metric, entry[str(c)][metric], direct)
                checked += not math.isnan(direct)
    assert checked >= 3 * 3 * (len(evaluated) - 1)
    for c in CLASSES:
        for metric in SURFACE:
            assert res["mean"][str(c)][metric] == float(np.nanmean([e[str(c)][metric] for e in res["all"]]))


def test_debug_false_writes_no_temporary_folder(dev, tmp_path):
    from cineflow import evaluation as E
    from cineflow import postprocessing as PP
    fx, js = fixture("B")
    base = str(tmp_path)
    names = write_tree(base, fx)
    pairs = [(os.path.join(base, "validation_raw", n), os.path.join(base, "gt", n)) for n in names]
    E.aggregate_scores(pairs, labels=CLASSES, json_output_file=os.path.join(base, "validation_raw", "summary.json"), advanced=True)
    before = set(os.listdir(base))
    PP.determine_postprocessing(base, os.path.join(base, "gt"), debug=False, log_function=lambda *a: None, pp_filename="pp.json")
    assert set(os.listdir(base)) - before == {"validation_final", "pp.json"}
    with open(os.path.join(base, "pp.json")) as f:
        assert json.load(f)["for_which_classes"] == js["postprocessing"]["for_which_classes"]
    assert np.array_equal(read_stack(os.path.join(base, "validation_final"), names), fx["final"])
    assert set(PP.LAST_TIMING) == {"read_s", "wall_s"}


def test_to_validate_list_replaces_the_u_rule(dev, tmp_path):
    """to_validate_list names the evaluated files; with every evaluated file of folder A named it decides as the `_u` rule does"""
    from cineflow import postprocessing as PP
    fx, js = fixture("A")
    base = str(tmp_path)
    names = write_tree(base, fx)
    with open(os.path.join(base, "validation_raw", "summary.json"), "w") as f:
        json.dump({"results": js["summary_raw"]}, f)
    PP.determine_postprocessing(base, os.path.join(base, "gt"), debug=False, log_function=lambda *a: None,
                                to_validate_list=[n for n in names if "_u" not in n])
    with open(os.path.join(base, "postprocessing.json")) as f:
        got = json.load(f)
    assert got["for_which_classes"] == js["postprocessing"]["for_which_classes"]
    assert got["dc_per_class_pp_per_class"] == js["postprocessing"]["dc_per_class_pp_per_class"]


def test_consolidate_folds_on_a_two_fold_tree(dev, tmp_path):
    from cineflow import evaluation as E
    from cineflow import postprocessing as PP
    from cineflow.nifti import write_nifti
    fx, js = fixture("E")
    base = str(tmp_path)
    names = [str(n) for n in fx["names"]]
    os.makedirs(os.path.join(base, "gt_niftis"))
    for n, p, g, fold in zip(names, fx["pred"], fx["gt"], fx["fold"]):
        raw = os.path.join(base, "fold_%d" % fold, "validation_raw")
        os.makedirs(raw, exist_ok=True)
        write_nifti(os.path.join(raw, n), p, SPACING)
        write_nifti(os.path.join(base, "gt_niftis", n), g, SPACING)
    for fold in (0, 1):
        raw = os.path.join(base, "fold_%d" % fold, "validation_raw")
        members = [n for n, f in zip(names, fx["fold"]) if f == fold]
        E.aggregate_scores([(os.path.join(raw, n), os.path.join(base, "gt_niftis", n)) for n in members], labels=CLASSES,
                           json_output_file=os.path.join(raw, "summary.json"), advanced=True)
    PP.consolidate_folds(base, folds=(0, 1))
    with open(os.path.join(base, "postprocessing.json")) as f:
        got = json.load(f)
    want = js["postprocessing"]
    for key in ("for_which_classes", "min_valid_object_sizes", "num_samples", "validation_raw", "validation_final", "dc_per_class_raw",
                "dc_per_class_pp_all", "dc_per_class_pp_per_class"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["validation_raw"] == "cv_niftis_raw" and got["validation_final"] == "cv_niftis_postprocessed"
    assert np.array_equal(read_stack(os.path.join(base, "cv_niftis_postprocessed"), names), fx["final"])
    for key, folder in (("raw", "cv_niftis_raw"), ("final", "cv_niftis_postprocessed")):
        with open(os.path.join(base, folder, "summary.json")) as f:
            assert_results_equal(json.load(f)["results"], js["summary_" + key], "E " + key)


def test_the_written_json_is_accepted_by_ensemble_predictions(runs, tmp_path):
    """merge(..., postprocessing_file=) with folder D's json (a joint region plus a single class, with size thresholds) on one-hot
    softmaxes of folder D's predictions gives folder D's final volumes -- through the export path's own kernels"""
    from cineflow import ensemble_predictions as EP
    base, names, _ = runs("D")
    fx, _ = fixture("D")
    folder = tmp_path / "member"
    folder.mkdir()
    for n, p in zip(names, fx["pred"]):
        onehot = (p[None] == np.arange(4, dtype=np.uint8)[:, None, None, None]).astype(np.float16)
        np.savez_compressed(str(folder / (n[:-7] + ".npz")), softmax=onehot)
        with open(str(folder / (n[:-7] + ".pkl")), "wb") as f:
            pickle.dump({"size_after_cropping": tuple(p.shape), "original_size_of_raw_data": np.array(p.shape), "itk_spacing": SPACING,
                         "itk_origin": (0.0, 0.0, 0.0), "itk_direction": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}, f)
    out = tmp_path / "out"
    EP.merge([str(folder)], str(out), 2, postprocessing_file=os.path.join(base, "postprocessing.json"))
    assert np.array_equal(read_stack(str(out / "not_postprocessed"), names), fx["pred"])
    assert np.array_equal(read_stack(str(out), names), fx["final"])
    assert os.path.isfile(str(out / "postprocessing.json"))
