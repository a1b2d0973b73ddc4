"""cineflow.evaluation.Evaluator on the device against counts taken with numpy: the routes the folder fixtures do not reach -- a subset of
the labels present (the histogram must still see the other labels as "not this label"), a label value the histogram cannot place,
`rv_rejection`, a joint region (tuple label), label files stored as float, to_array / to_pandas.  Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = ("Dice", "Jaccard", "Precision", "Recall", "Accuracy", "False Positive Rate", "Total Positives Test", "Total Positives Reference")


def volumes(top=3):
    rng = np.random.default_rng(3)
    shape = (5, 21, 33)
    ref = rng.integers(0, top + 1, shape).astype(np.uint8)
    test = np.where(rng.random(shape) < 0.7, ref, rng.integers(0, top + 1, shape)).astype(np.uint8)
    return test, ref


def numpy_scores(t, r):
    """the expressions of nnunet/evaluation/metrics.py on numpy masks"""
    tp, fp, fn, tn = int((t & r).sum()), int((t & ~r).sum()), int((~t & r).sum()), int((~t & ~r).sum())
    return {"Dice": float(2. * tp / (2 * tp + fp + fn)), "Jaccard": float(tp / (tp + fp + fn)), "Precision": float(tp / (tp + fp)),
            "Recall": float(tp / (tp + fn)), "Accuracy": float((tp + tn) / (tp + fp + tn + fn)), "False Positive Rate": 1 - float(tn / (tn + fp)),
            "Total Positives Test": tp + fp, "Total Positives Reference": tp + fn}


def check(result, name, t, r):
    want = numpy_scores(t, r)
    for m in RATIOS:
        assert result[name][m] == want[m], (name, m, result[name][m], want[m])


@pytest.mark.parametrize("labels", [[1], [1, 2], [2, 3], [0, 1, 2, 3]])
def test_a_subset_of_the_labels_present_scores_like_per_label_masks(dev, labels):
    from cineflow.evaluation import Evaluator
    test, ref = volumes()
    res = Evaluator(labels=labels).evaluate(test, ref)
    assert list(res) == [str(l) for l in labels]
    for l in labels:
        check(res, str(l), test == l, ref == l)


def test_a_label_the_histogram_cannot_place_takes_the_per_label_route(dev):
    from cineflow.evaluation import Evaluator
    test, ref = volumes()
    test, ref = test.copy(), ref.copy()
    test[0, :4, :4] = 40
    ref[0, :2, :4] = 40
    ref[0, 2:6, :4] = 200
    res = Evaluator(labels=[1, 3, 40, 200]).evaluate(test, ref)
    for l in (1, 3, 40):
        check(res, str(l), test == l, ref == l)
    assert res["200"]["Total Positives Reference"] == 16 and res["200"]["Total Positives Test"] == 0


def test_rv_rejection_joint_regions_float_files_and_tables(dev):
    from cineflow.evaluation import Evaluator
    test, ref = volumes()
    res = Evaluator(labels=[1, 2], rv_rejection=True).evaluate(test, ref)
    check(res, "1", (test == 1)[2:], (ref == 1)[2:])
    check(res, "2", test == 2, ref == 2)
    named = Evaluator(labels={1: "RV", (2, 3): "LV+MYO"}, rv_rejection=True)
    res = named.evaluate(test.astype(np.float32), ref.astype(np.float64))                 # label files are often stored as float
    check(res, "RV", test == 1, ref == 1)                                                # (no rv_rejection for named labels, as in the reference)
    check(res, "LV+MYO", (test == 2) | (test == 3), (ref == 2) | (ref == 3))
    table = named.to_array()
    columns = sorted(res["RV"])
    assert table.shape == (2, len(columns)) and table.dtype == np.float32
    assert table[1, columns.index("Dice")] == np.float32(res["LV+MYO"]["Dice"])
    frame = named.to_pandas()
    assert list(frame.index) == ["RV", "LV+MYO"] and list(frame.columns) == columns
    assert frame.loc["RV", "Jaccard"] == np.float32(res["RV"]["Jaccard"])
    with pytest.raises(ValueError):
        from cineflow.evaluation import label_volume_u8
        label_volume_u8(test + 0.5, "half labels")
