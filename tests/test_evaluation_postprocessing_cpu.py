"""CPU tests (no GPU) of cineflow.evaluation and cineflow.postprocessing: label handling of the Evaluator, the summary.json layout and id
hash of aggregate_scores (with an evaluator that needs no device), the folder assertions of evaluate_folder / consolidate_folds, the
load_postprocessing round trip of a written postprocessing.json, the command lines, and the committed fixture's own claims."""
import collections
import hashlib
import inspect
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postprocessing")


def test_evaluator_label_handling():
    from cineflow.evaluation import Evaluator, NiftiEvaluator
    e = Evaluator()
    assert e.metrics == Evaluator.default_metrics and e.metrics is not Evaluator.default_metrics
    assert e.advanced_metrics == ["Hausdorff Distance", "Hausdorff Distance 95", "Avg. Symmetric Surface Distance"]
    assert len(Evaluator.default_metrics) == 13 and "Avg. Surface Distance" not in Evaluator.default_advanced_metrics
    e.set_labels({1: "RV", (2, 3): "LV+MYO"})
    assert isinstance(e.labels, collections.OrderedDict) and list(e.labels.values()) == ["RV", "LV+MYO"]
    e.set_labels({3, 1})
    assert sorted(e.labels) == [1, 3] and isinstance(e.labels, list)
    e.set_labels(np.array([2, 1]))
    assert e.labels == [2, 1]
    e.set_labels((1, 2))
    assert e.labels == (1, 2)
    with pytest.raises(TypeError):
        e.set_labels("12")
    with pytest.raises(ValueError):
        Evaluator().construct_labels()
    e = Evaluator(test=np.array([[0, 2], [5, 2]]), reference=np.array([[0, 1], [1, 1]]))
    assert e.labels == [0, 1, 2, 5] and all(type(v) is int for v in e.labels)
    e = Evaluator(reference=np.array([0, 3]))
    e.construct_labels()
    assert e.labels == [0, 3]
    e.set_metrics({"Dice"})
    assert e.metrics == ["Dice"]
    e.add_metric("Jaccard")
    e.add_metric("Dice")
    assert e.metrics == ["Dice", "Jaccard"]
    with pytest.raises(TypeError):
        e.set_metrics("Dice")
    with pytest.raises(ValueError):
        Evaluator().evaluate()
    assert issubclass(NiftiEvaluator, Evaluator) and NiftiEvaluator(rv_rejection=True).rv_rejection is True
    for name in ("set_test", "set_reference", "set_labels", "construct_labels", "set_metrics", "add_metric", "evaluate", "to_dict", "to_array",
                 "to_pandas"):
        assert callable(getattr(Evaluator, name))


def test_signatures_follow_the_reference():
    from cineflow import evaluation as E
    from cineflow import postprocessing as PP
    assert list(inspect.signature(E.aggregate_scores).parameters) == [
        "test_ref_pairs", "evaluator", "labels", "nanmean", "json_output_file", "json_name", "json_description", "json_author", "json_task",
        "num_threads", "metadata_list", "rv_rejection", "nb_threads", "binary", "metric_kwargs"]
    sig = inspect.signature(PP.determine_postprocessing)
    assert list(sig.parameters) == ["base", "gt_labels_folder", "raw_subfolder_name", "temp_folder", "final_subf_name", "processes", "dice_threshold",
                                    "debug", "advanced_postprocessing", "pp_filename", "log_function", "metadata_list", "binary", "to_validate_list",
                                    "nb_threads"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["raw_subfolder_name"], d["temp_folder"], d["final_subf_name"], d["pp_filename"]) == ("validation_raw", "temp", "validation_final",
                                                                                                   "postprocessing.json")
    assert d["processes"] == 1 and d["dice_threshold"] == 0 and d["debug"] is True and d["advanced_postprocessing"] is False and d["nb_threads"] == 1
    assert d["log_function"] is print and d["metadata_list"] is None and d["binary"] is False and d["to_validate_list"] is None
    assert list(inspect.signature(PP.consolidate_folds).parameters) == ["output_folder_base", "validation_folder_name", "advanced_postprocessing", "folds"]
    assert inspect.signature(PP.consolidate_folds).parameters["folds"].default == (0, 1, 2, 3, 4)
    assert list(inspect.signature(PP.apply_postprocessing_to_folder).parameters) == ["input_folder", "output_folder", "for_which_classes",
                                                                                     "min_valid_object_size", "num_processes"]
    a = E.build_parser().parse_args(["-ref", "r", "-pred", "p", "-l", "1", "2", "3"])
    assert (a.ref, a.pred, a.l) == ("r", "p", [1, 2, 3])
    assert PP.build_parser().parse_args(["-f", "x"]).f == "x"
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["-ref", "r"])


class TableEvaluator:
    """an evaluator that needs no device: scores come from a table keyed by the test name"""

    def __init__(self, table):
        self.table, self.labels, self.test = table, None, None

    def set_labels(self, labels):
        self.labels = labels

    def set_test(self, test):
        self.test = test

    def set_reference(self, reference, binary=False):
        self.reference = reference

    def evaluate(self, **kwargs):
        return collections.OrderedDict((str(l), collections.OrderedDict(self.table[self.test][l])) for l in self.labels)


def test_summary_json_layout_mean_rules_and_id_hash(tmp_path):
    from cineflow.evaluation import aggregate_scores
    nan = float("nan")
    table = {"a": {1: {"Dice": 0.5, "Total Positives Test": 4}, 2: {"Dice": nan, "Total Positives Test": 0}},
             "b": {1: {"Dice": 0.25, "Total Positives Test": 6}, 2: {"Dice": 1.0, "Total Positives Test": 2}}}
    out = str(tmp_path / "summary.json")
    meta = [{"patient": "p1", "1": "shadowed"}, {"patient": "p2"}]
    res = aggregate_scores([("a", "ra"), ("b", "rb")], evaluator=TableEvaluator(table), labels=[1, 2], json_output_file=out, json_name="n",
                           json_description="d", json_task="t", metadata_list=meta)
    assert list(res) == ["all", "mean"] and len(res["all"]) == 2
    assert res["all"][0]["test"] == "a" and res["all"][0]["reference"] == "ra" and res["all"][1]["patient"] == "p2"
    # a metadata key that shadows a label replaces that case's scores and keeps them out of the mean, as in the reference
    assert res["all"][0]["1"] == "shadowed"
    assert res["mean"]["1"] == {"Dice": 0.25, "Total Positives Test": 6.0}
    assert res["mean"]["2"] == {"Dice": 1.0, "Total Positives Test": 1.0}                # nanmean skips the NaN
    assert "patient" not in res["mean"] and "test" not in res["mean"]
    plain = aggregate_scores([("a", "ra"), ("b", "rb")], evaluator=TableEvaluator(table), labels=[1, 2], nanmean=False)
    assert np.isnan(plain["mean"]["2"]["Dice"]) and plain["mean"]["1"]["Dice"] == 0.375
    with open(out) as f:
        text = f.read()
    written = json.loads(text)
    assert list(json.loads(text, object_pairs_hook=collections.OrderedDict)) == sorted(written)           # save_json sorts keys, indent 4
    assert text.startswith('{\n    "author": "Fabian"')
    assert (written["name"], written["description"], written["task"], written["author"]) == ("n", "d", "t", "Fabian")
    body = collections.OrderedDict((k, written[k]) for k in ("name", "description", "timestamp", "task", "author"))
    body["results"] = res
    assert written["id"] == hashlib.md5(json.dumps(body).encode("utf-8")).hexdigest()[:12]


def test_aggregate_scores_for_experiment(tmp_path):
    from cineflow.evaluation import Evaluator, aggregate_scores_for_experiment
    scores = np.arange(2 * 3 * 13, dtype=np.float64).reshape(2, 3, 13)
    np.save(str(tmp_path / "s.npy"), scores)
    out = str(tmp_path / "o.json")
    d = aggregate_scores_for_experiment(str(tmp_path / "s.npy"), json_output_file=out)
    assert list(d["results"]["mean"]) == ["0", "1", "2"] and d["results"]["mean"]["1"][Evaluator.default_metrics[2]] == float(scores[:, 1, 2].mean())
    assert d["results"]["all"][1]["2"]["Dice"] == float(scores[1, 2, 1])
    with open(out) as f:
        assert json.load(f)["id"] == d["id"]


def _touch_nifti(path):
    from cineflow.nifti import write_nifti
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_nifti(path, np.zeros((1, 2, 2), np.uint8))


def test_evaluate_folder_refuses_folders_that_do_not_match(tmp_path):
    from cineflow.evaluation import evaluate_folder
    for n in ("a", "b"):
        _touch_nifti(str(tmp_path / "gt" / (n + ".nii.gz")))
    _touch_nifti(str(tmp_path / "pred" / "a.nii.gz"))
    with pytest.raises(AssertionError, match="files missing in folder_with_predictions"):
        evaluate_folder(str(tmp_path / "gt"), str(tmp_path / "pred"), (1, 2))
    _touch_nifti(str(tmp_path / "pred" / "b.nii.gz"))
    _touch_nifti(str(tmp_path / "pred" / "c.nii.gz"))
    with pytest.raises(AssertionError, match="files missing in folder_with_gts"):
        evaluate_folder(str(tmp_path / "gt"), str(tmp_path / "pred"), (1, 2))


def test_consolidate_folds_refuses_missing_folds_and_a_file_count_mismatch(tmp_path):
    from cineflow.postprocessing import collect_cv_niftis, consolidate_folds
    base = str(tmp_path)
    _touch_nifti(os.path.join(base, "fold_0", "validation_raw", "a.nii.gz"))
    with pytest.raises(RuntimeError, match=r"some folds are missing.*\[1, 2\]"):
        consolidate_folds(base, folds=(0, 1, 2))
    _touch_nifti(os.path.join(base, "fold_1", "validation_raw", "b.nii.gz"))
    for n in ("a", "b", "c"):
        _touch_nifti(os.path.join(base, "gt_niftis", n + ".nii.gz"))
    os.makedirs(os.path.join(base, "cv_niftis_raw", "stale"))
    with pytest.raises(AssertionError, match="trained all the folds"):
        consolidate_folds(base, folds=(0, 1))
    assert sorted(os.listdir(os.path.join(base, "cv_niftis_raw"))) == ["a.nii.gz", "b.nii.gz"]             # collected afresh, the stale folder is gone
    collect_cv_niftis(base, os.path.join(base, "again"), folds=(1,))
    assert os.listdir(os.path.join(base, "again")) == ["b.nii.gz"]


def test_determine_postprocessing_needs_the_raw_summary(tmp_path):
    from cineflow.postprocessing import determine_postprocessing
    os.makedirs(str(tmp_path / "validation_raw"))
    with pytest.raises(AssertionError, match="does not contain a summary.json"):
        determine_postprocessing(str(tmp_path), str(tmp_path / "gt"))
    with open(str(tmp_path / "validation_raw" / "summary.json"), "w") as f:
        json.dump({"results": {"all": [], "mean": {"0": {}, "17": {}}}}, f)
    with pytest.raises(ValueError, match="labels below 16"):
        determine_postprocessing(str(tmp_path), str(tmp_path / "gt"))


def test_written_postprocessing_json_round_trips_through_load_postprocessing(tmp_path):
    """the layout determine_postprocessing writes (connected_components.py:406-437) read back by the consumer of the file"""
    from cineflow.evaluation import save_json
    from cineflow.export import load_postprocessing
    classes = [1, 2, 3]
    pp = {"dc_per_class_raw": {"1": 0.5}, "dc_per_class_pp_all": {"1": 0.6}, "dc_per_class_pp_per_class": {}, "for_which_classes": [classes, 2],
          "min_valid_object_sizes": str({tuple(classes): 3900.0, 2: 1500.0}), "num_samples": 7, "validation_raw": "validation_raw",
          "validation_final": "validation_final"}
    path = str(tmp_path / "postprocessing.json")
    save_json(pp, path)
    fwc, sizes = load_postprocessing(path)
    assert fwc == [[1, 2, 3], 2] and sizes == {(1, 2, 3): 3900.0, 2: 1500.0}
    pp["min_valid_object_sizes"] = str(None)
    save_json(pp, path)
    assert load_postprocessing(path) == ([[1, 2, 3], 2], None)


@pytest.mark.parametrize("tag", ["A", "B", "C", "D", "E"])
def test_fixture_is_what_its_report_says(tag):
    """the committed folders decide differently, hold the `_u` file and the NaN case, and their final volumes follow from their json through the
    oracle's filter (so the fixture cannot drift from its own decisions)"""
    import ast
    from oracle import ops as OO
    fx = np.load(os.path.join(GOLDEN, tag + ".npz"))
    with open(os.path.join(GOLDEN, "decisions.json")) as f:
        pp = json.load(f)[tag]
    dice_raw = fx["summary_raw"][:-1, :, [str(m) for m in fx["summary_metrics"]].index("Dice")]          # [cases, classes]
    fwc = pp["for_which_classes"]
    want = {"A": [[1, 2, 3], 2], "B": [1], "C": [], "D": [[1, 2, 3], 2], "E": [[1, 2, 3]]}[tag]
    assert fwc == want
    names = [str(n) for n in fx["names"]]
    assert ("case_u07.nii.gz" in names) == (tag == "A")
    assert pp["num_samples"] == len([n for n in names if "_u" not in n]) == len(dice_raw)
    if tag == "A":
        assert np.isnan(dice_raw[:, 2]).any() and not np.isnan(dice_raw[:, :2]).any()
    if tag == "B":
        assert pp["dc_per_class_pp_all"]["3"] < pp["dc_per_class_raw"]["3"]
    sizes = ast.literal_eval(pp["min_valid_object_sizes"])
    assert (sizes is not None) == (tag == "D")
    vpv = 1.25 * 1.25 * 8.0
    for pred, final in zip(fx["pred"], fx["final"]):
        got, _, _ = OO.remove_all_but_the_largest_connected_component(pred.copy(), [tuple(c) if isinstance(c, list) else c for c in fwc], vpv, sizes)
        assert np.array_equal(got, final)
    with open(os.path.join(os.path.dirname(GOLDEN), "PIN_REPORT_postprocessing.txt")) as f:
        assert "parity unpinned" in f.read()
