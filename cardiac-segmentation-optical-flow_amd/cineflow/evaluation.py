"""Folder evaluation on the device: the interface of nnunet/evaluation/evaluator.py:31-510 (Evaluator, NiftiEvaluator, run_evaluation,
aggregate_scores, aggregate_scores_for_experiment, evaluate_folder; same names, argument lists, defaults and summary.json layout), restated.

The numbers come from cineflow.metrics.  All confusion-type metrics of a case come from ONE cf_label_confusion launch whose 16 x 16 histogram
is sliced per label; tuple labels (joint regions), `rv_rejection`'s label 1 and volumes holding a label value the histogram cannot place
take one ConfusionMatrix per label instead.  Files go through cineflow.nifti; a thread pool reads and inflates the next cases while the
device works on the current one, and only this process opens the GPU.  The surface metrics search the two borders all-pairs
(--surface pairs), or read HD, HD95 and ASSD of all histogram labels of a case from one exact distance-transform visit (--surface edt:
cineflow.metrics.label_surface_edt_table, linear in the volume -- the route for 3-D organs); auto picks by the size of the borders.

    python -m cineflow.evaluation -ref GT_FOLDER -pred PRED_FOLDER -l 1 2 3 [--surface auto|pairs|edt] [--surface_dice MM]

Region-based evaluation (nnunet/evaluation/region_based_evaluation.py: get_brats_regions, get_KiTS_regions, create_region_from_mask,
evaluate_case, evaluate_regions; same names and summary.csv layout), restated: a region is a set of label values, each case is read once,
its K x K label confusion is counted by one cf_label_confusion launch, and every region's |P n G|, |P| and |G| are sums of its cells.
Dice = 2 |P n G| / (|P| + |G|), NaN when both are empty -- the value medpy's metric.dc gives; medpy and SimpleITK are not used, so parity
of summary.csv with the reference's file is by this restatement, not pinned against a run of it.

    python -m cineflow.evaluation --regions brats|kits|JSON -ref GT_FOLDER -pred PRED_FOLDER
"""
import collections
import hashlib
import inspect
import json
import warnings
from collections import OrderedDict
from datetime import datetime
from os.path import join

import numpy as np

from . import metrics
from ._lib import lib                                              # noqa: F401  (every launch is metrics'; call counters patch the name here too)
from .folder_io import Loaded, load_volume, read_ahead, save_json, subfiles
from .metrics import ALL_METRICS, ConfusionMatrix, label_volume_u8

HIST_K = 16
SURFACE_DICE = "Normalized Surface Dice"
# the surface metrics a label_surface_edt_table entry answers, and the entry's key for each
TABLE_COLUMNS = {"Hausdorff Distance": "hd", "Hausdorff Distance 95": "hd95", "Avg. Symmetric Surface Distance": "assd",
                 "Avg. Surface Distance": "asd_test_to_ref"}

# a test volume whose label confusion against its reference is already counted (cineflow.ops.ensemble_pairs counts it while it writes the
# labels): (file name it stands for, hist [16,16] of counts[test label, reference label], voxels).  Neither file is read.
Counted = collections.namedtuple("Counted", "path hist n")


class _SlicedMatrix(ConfusionMatrix):
    """ConfusionMatrix of `test == label` vs `reference == label` whose counts are one row and one column of the label histogram.  The two
    masks are only built when a surface metric asks for them."""

    def __init__(self, hist, label, n, test_t, ref_t):
        tp = int(hist[label, label])
        fp, fn = int(hist[label, :].sum()) - tp, int(hist[:, label].sum()) - tp
        self.tp, self.fp, self.fn, self.tn, self.size = tp, fp, fn, n - tp - fp - fn, n
        self.test_empty, self.test_full = tp + fp == 0, tp + fp == n
        self.reference_empty, self.reference_full = tp + fn == 0, tp + fn == n
        self._label, self._test_t, self._ref_t = label, test_t, ref_t

    test = property(lambda self: self._test_t == self._label)
    reference = property(lambda self: self._ref_t == self._label)


class Evaluator:
    """Scores a test segmentation against a reference one, label by label.  `labels`: a list / tuple / set / array of label values, or a
    dict {label value or tuple of values (a joint region): name}; without it the labels are the values found in the two volumes."""

    default_metrics = ["False Positive Rate", "Dice", "Jaccard", "Precision", "Recall", "Accuracy", "False Omission Rate",
                       "Negative Predictive Value", "False Negative Rate", "True Negative Rate", "False Discovery Rate", "Total Positives Test",
                       "Total Positives Reference"]
    default_advanced_metrics = ["Hausdorff Distance", "Hausdorff Distance 95", "Avg. Symmetric Surface Distance"]

    def __init__(self, test=None, reference=None, labels=None, metrics=None, advanced_metrics=None, nan_for_nonexisting=True,
                 rv_rejection=False):
        self.test = self.reference = self.labels = self.result = None
        self.confusion_matrix = ConfusionMatrix()
        self.nan_for_nonexisting = nan_for_nonexisting
        self.rv_rejection = rv_rejection
        self.metrics = list(self.default_metrics if metrics is None else metrics)
        self.advanced_metrics = list(self.default_advanced_metrics if advanced_metrics is None else advanced_metrics)
        self.set_reference(reference)
        self.set_test(test)
        if labels is not None:
            self.set_labels(labels)
        elif test is not None and reference is not None:
            self.construct_labels()

    def set_test(self, test):
        self.test = test

    def set_reference(self, reference):
        self.reference = reference

    def set_labels(self, labels):
        if isinstance(labels, dict):
            self.labels = OrderedDict(labels)
        elif isinstance(labels, (set, np.ndarray)):
            self.labels = list(labels)
        elif isinstance(labels, (list, tuple)):
            self.labels = labels
        else:
            raise TypeError("Can only handle dict, list, tuple, set & numpy array, but input is of type {}".format(type(labels)))

    def construct_labels(self):
        """labels = the values present in the test and reference volumes (the reference volume alone when there is no test)"""
        given = [v for v in (self.test, self.reference) if v is not None]
        if not given:
            raise ValueError("No test or reference segmentations.")
        self.labels = [int(v) for v in np.unique(np.concatenate([np.unique(v) for v in given]))]

    def set_metrics(self, metrics):
        if isinstance(metrics, set):
            metrics = list(metrics)
        elif not isinstance(metrics, (list, tuple, np.ndarray)):
            raise TypeError("Can only handle list, tuple, set & numpy array, but input is of type {}".format(type(metrics)))
        self.metrics = metrics

    def add_metric(self, metric):
        if metric not in self.metrics:
            self.metrics.append(metric)

    def _metric_functions(self, names):
        """ALL_METRICS, or -- evaluator.py:171-186 -- a function of that name in a local scope of one of the callers"""
        funcs = {}
        frames = None
        for name in names:
            if name in ALL_METRICS:
                funcs[name] = ALL_METRICS[name]
                continue
            frames = inspect.getouterframes(inspect.currentframe()) if frames is None else frames
            found = [f[0].f_locals[name] for f in frames if name in f[0].f_locals]
            if not found:
                raise NotImplementedError("Metric {} not implemented.".format(name))
            funcs[name] = found[0]
        return funcs

    def _histogram(self):
        """One cf_label_confusion launch for the case -> (hist [16,16] numpy, test_t, ref_t, n), or None when the volumes do not fit it:
        values outside 0..255, or a voxel with a label >= 16 in either volume (the kernel counts those in one overflow bin, so no row or
        column sum would be complete)."""
        try:
            test_t, ref_t = label_volume_u8(self.test, "test"), label_volume_u8(self.reference, "reference")
        except ValueError:
            return None
        hist, overflow = metrics.label_histogram(test_t, ref_t, HIST_K)
        return None if overflow else (hist, test_t, ref_t, test_t.numel())

    def _per_label_matrix(self, label, joint, cut_rv):
        """the per-label route: one ConfusionMatrix on masks (a joint region is the union of its labels, evaluator.py:204-210; rv_rejection
        scores label 1 without the first two slices, evaluator.py:223-225)"""
        values = list(label) if joint else [label]
        test = np.isin(np.asarray(self.test), values)
        reference = np.isin(np.asarray(self.reference), values)
        if cut_rv:
            test, reference = test[2:], reference[2:]
        self.confusion_matrix.set_test(test)
        self.confusion_matrix.set_reference(reference)
        return self.confusion_matrix

    def _surface_table(self, histogram, labels, surface, voxel_spacing):
        """One label_surface_edt_table visit for the case's histogram labels -> {label: its entry}, or None when the route is `auto` and no
        label's two borders hold more than metrics.EDT_AUTO_PAIRS pairs (the per-label search then scores the case exactly as before).
        `auto` first asks the histogram: a label's border voxels are at most its voxels, so a case whose voxel products all stay under
        the constant never pays for the visit."""
        hist, test_t, ref_t, _ = histogram
        labels = sorted(set(labels))
        voxels = [(int(hist[c, :].sum()), int(hist[:, c].sum())) for c in labels]
        if surface != "edt" and all(a * b <= metrics.EDT_AUTO_PAIRS for a, b in voxels):
            return None
        table = metrics.label_surface_edt_table(test_t, ref_t, labels, voxel_spacing, capacity=sum(a + b for a, b in voxels))
        if surface != "edt" and all(e["n_test"] * e["n_ref"] <= metrics.EDT_AUTO_PAIRS for e in table.values()):
            return None
        return table

    def evaluate(self, test=None, reference=None, advanced=False, surface=None, surface_dice_threshold=None, histogram=None, **metric_kwargs):
        """-> OrderedDict {label name: {metric: value}}; with advanced=True the surface metrics are added.  surface: how their distances
        are found -- "pairs" (the all-pairs search), "edt" (the exact distance transform: the histogram labels of the case in one
        label_surface_edt_table visit, the other labels one by one), None / "auto" ("pairs" unless some label's borders hold more than
        metrics.EDT_AUTO_PAIRS pairs).  surface_dice_threshold (mm): adds "Normalized Surface Dice" to every label.
        histogram: (hist [16,16] of counts[test label, reference label], voxels) of the case, counted already -- the volumes are then not
        needed and nothing is launched; it answers plain labels below 16 and the confusion-type metrics only (anything else is refused)."""
        if surface not in (None, "auto", "pairs", "edt"):
            raise ValueError("surface must be one of auto, pairs, edt, got %r" % (surface,))
        surface = None if surface == "auto" else surface
        if histogram is not None:
            return self._evaluate_counted(histogram, advanced, surface_dice_threshold, metric_kwargs)
        if test is not None:
            self.set_test(test)
        if reference is not None:
            self.set_reference(reference)
        if self.test is None or self.reference is None:
            raise ValueError("Need both test and reference segmentations.")
        if self.labels is None:
            self.construct_labels()
        self.metrics.sort()
        wanted = list(self.metrics) + ([m for m in self.advanced_metrics if m not in self.metrics] if advanced else [])
        funcs = self._metric_functions(wanted)
        metric_kwargs.setdefault("reproducible", True)            # summary values must not depend on the order the border voxels were found in

        named = isinstance(self.labels, dict)
        items = list(self.labels.items()) if named else [(l, l) for l in self.labels]
        routes = []
        for label, name in items:
            joint = hasattr(label, "__iter__")
            if joint and not named:
                raise TypeError("joint regions (tuple labels) need a dict of labels {tuple: name}")
            cut_rv = bool(self.rv_rejection) and not named and label == 1
            routes.append((label, name, joint, cut_rv, not joint and not cut_rv and 0 <= int(label) < HIST_K))
        histogram = self._histogram() if any(r[4] for r in routes) else None

        if surface is not None:
            metric_kwargs["method"] = surface
        if surface_dice_threshold is not None:
            wanted.append(SURFACE_DICE)
            funcs[SURFACE_DICE] = metrics.normalized_surface_dice_metric
            metric_kwargs["threshold"] = float(surface_dice_threshold)
        from_table = [m for m in wanted if funcs[m] is ALL_METRICS.get(m) and m in TABLE_COLUMNS or m == SURFACE_DICE]
        table = None
        if histogram is not None and from_table and surface != "pairs":
            table = self._surface_table(histogram, [int(r[0]) for r in routes if r[4]], surface, metric_kwargs.get("voxel_spacing"))

        self.result = OrderedDict()
        for label, name, joint, cut_rv, sliced in routes:
            sliced = sliced and histogram is not None
            cm = _SlicedMatrix(histogram[0], int(label), histogram[3], histogram[1], histogram[2]) if sliced \
                else self._per_label_matrix(label, joint, cut_rv)
            entry = table[int(label)] if sliced and table is not None else None
            scores = OrderedDict()
            for m in wanted:
                if entry is not None and m in from_table:
                    scores[m] = self._from_table(m, entry, cm, metric_kwargs.get("threshold"))
                else:
                    scores[m] = funcs[m](confusion_matrix=cm, nan_for_nonexisting=self.nan_for_nonexisting, **metric_kwargs)
            self.result[str(name)] = scores
        return self.result

    def _evaluate_counted(self, histogram, advanced, surface_dice_threshold, metric_kwargs):
        """evaluate() from a ready histogram: the same _SlicedMatrix per label and the same metric functions, no volume and no launch"""
        hist, n = np.asarray(histogram[0]), int(histogram[1])
        if hist.shape != (HIST_K, HIST_K):
            raise ValueError("histogram must be [%d,%d] counts[test label, reference label], got %s" % (HIST_K, HIST_K, hist.shape))
        if advanced or surface_dice_threshold is not None:
            raise ValueError("a ready histogram answers the confusion-type metrics only: surface metrics need the volumes")
        if self.labels is None:
            raise ValueError("a ready histogram needs the labels to score")
        named = isinstance(self.labels, dict)
        items = list(self.labels.items()) if named else [(l, l) for l in self.labels]
        for label, _ in items:
            if hasattr(label, "__iter__") or not 0 <= int(label) < HIST_K or (bool(self.rv_rejection) and not named and label == 1):
                raise ValueError("label %r is not answered by the histogram (joint region, rv_rejection's label 1, or a value >= %d)"
                                 % (label, HIST_K))
        self.metrics.sort()
        funcs = self._metric_functions(list(self.metrics))
        metric_kwargs.setdefault("reproducible", True)
        self.result = OrderedDict()
        for label, name in items:
            cm = _SlicedMatrix(hist, int(label), n, None, None)
            self.result[str(name)] = OrderedDict((m, funcs[m](confusion_matrix=cm, nan_for_nonexisting=self.nan_for_nonexisting, **metric_kwargs))
                                                 for m in self.metrics)
        return self.result

    def _from_table(self, metric, entry, cm, threshold):
        """a surface metric of one label from its label_surface_edt_table entry, under _surface_metric's existence rule"""
        if any(cm.get_existence()):
            return float("NaN") if self.nan_for_nonexisting else 0
        if metric == SURFACE_DICE:
            return metrics.surface_dice_from_distances(entry["d_test_to_ref"], entry["d_ref_to_test"], threshold)
        return entry[TABLE_COLUMNS[metric]]

    def to_dict(self):
        if self.result is None:
            self.evaluate()
        return self.result

    def _names_and_columns(self):
        names = [str(v) for v in (self.labels.values() if isinstance(self.labels, dict) else self.labels)]
        return names, sorted(self.to_dict()[names[0]])

    def to_array(self):
        """float32 [labels, metrics], metrics in sorted order"""
        names, columns = self._names_and_columns()
        return np.array([[self.result[n][m] for m in columns] for n in names], dtype=np.float32)

    def to_pandas(self):
        import pandas as pd
        names, columns = self._names_and_columns()
        return pd.DataFrame(self.to_array(), index=names, columns=columns)


class NiftiEvaluator(Evaluator):
    """Evaluator on files (cineflow.nifti); a `Loaded` volume is taken as it is, which is how aggregate_scores reads ahead."""

    def __init__(self, *args, **kwargs):
        self.test_nifti = self.reference_nifti = None
        super().__init__(*args, **kwargs)

    def set_test(self, test):
        self.test_nifti = None if test is None else test if isinstance(test, Loaded) else load_volume(test)
        super().set_test(None if test is None else self.test_nifti.array)

    def set_reference(self, reference, binary=False):
        self.reference_nifti = None if reference is None else reference if isinstance(reference, Loaded) else load_volume(reference)
        mask = None if reference is None else self.reference_nifti.array
        if binary and mask is not None:
            mask = (mask > 0).astype(mask.dtype)
        super().set_reference(mask)

    def evaluate(self, test=None, reference=None, voxel_spacing=None, **metric_kwargs):
        if voxel_spacing is None:                                  # array axes are (z, y, x), itk spacing is (x, y, z): evaluator.py:311
            voxel_spacing = np.array(self.test_nifti.props["itk_spacing"])[::-1]
        metric_kwargs["voxel_spacing"] = voxel_spacing
        return super().evaluate(test, reference, **metric_kwargs)


def _name(x):
    return x.path if isinstance(x, (Loaded, Counted)) else x


def run_evaluation(args):
    """one case: (test, reference, evaluator, metric_kwargs, metadata, binary) -> its scores plus file names and metadata"""
    test, ref, evaluator, metric_kwargs, metadata, binary = args
    if isinstance(test, Counted):                                  # scored from its ready histogram: neither file is read
        scores = Evaluator.evaluate(evaluator, histogram=(test.hist, test.n), **metric_kwargs)
    else:
        evaluator.set_test(test)
        evaluator.set_reference(ref, binary)
        if evaluator.labels is None:
            evaluator.construct_labels()
        scores = evaluator.evaluate(**metric_kwargs)
    for key, source in (("test", test), ("reference", ref)):
        if isinstance(_name(source), str):
            scores[key] = _name(source)
    scores.update(metadata)
    return scores


def _summary(name, description, task, author, results):
    """the summary.json document; its id is the md5 of the document without the id (evaluator.py:414-424)"""
    doc = OrderedDict([("name", name), ("description", description), ("timestamp", str(datetime.today())), ("task", task), ("author", author),
                       ("results", results)])
    doc["id"] = hashlib.md5(json.dumps(doc).encode("utf-8")).hexdigest()[:12]
    return doc


def aggregate_scores(test_ref_pairs, evaluator=NiftiEvaluator, labels=None, nanmean=True, json_output_file=None, json_name="",
                     json_description="", json_author="Fabian", json_task="", num_threads=2, metadata_list=None, rv_rejection=False,
                     nb_threads=1, binary=False, **metric_kwargs):
    """Scores every (test, reference) pair -- file names, `Loaded` volumes, or a `Counted` test with its reference's file name -- and returns {"all": [scores of each case], "mean": {label:
    {metric: mean over the cases}}} (nanmean: NaN cases do not count); with json_output_file the summary.json is written.  labels: a list of
    ints or a dict int -> name.  num_threads / nb_threads: reader threads (the larger of the two); the device work stays in this process."""
    if isinstance(evaluator, type):
        evaluator = evaluator(rv_rejection=rv_rejection)
    if labels is not None:
        evaluator.set_labels(labels)
    tests, refs = [p[0] for p in test_ref_pairs], [p[1] for p in test_ref_pairs]
    metadata_list = [{}] * len(refs) if metadata_list is None else metadata_list
    count = min(len(tests), len(metadata_list))                    # (the reference zips the lists: the shortest one ends the run)

    readers = max(1, min(16, max(int(nb_threads or 1), int(num_threads or 1))))
    prefetch = isinstance(evaluator, NiftiEvaluator)
    # read ahead of case i: both files, or nothing for a Counted test (its reference is not read either); Loaded entries pass through
    groups = [(tests[i], refs[i]) if prefetch and not isinstance(tests[i], Counted) else () for i in range(count)]
    cases = read_ahead(groups, lambda f: load_volume(f) if isinstance(f, str) else f, depth=readers, readers=readers)
    per_case = [run_evaluation((*(pair or (tests[i], refs[i])), evaluator, metric_kwargs, metadata_list[i], binary))
                for i, (_, pair) in enumerate(cases)]

    mean_of = np.nanmean if nanmean else np.mean
    collected = OrderedDict()
    for scores, metadata in zip(per_case, metadata_list):
        for label, by_metric in scores.items():
            if label in ("test", "reference") or label in metadata:
                continue
            for metric, value in by_metric.items():
                collected.setdefault(label, OrderedDict()).setdefault(metric, []).append(value)
    results = OrderedDict([("all", per_case),
                           ("mean", OrderedDict((label, OrderedDict((m, float(mean_of(v))) for m, v in by_metric.items()))
                                                for label, by_metric in collected.items()))])
    if json_output_file is not None:
        save_json(_summary(json_name, json_description, json_task, json_author, results), json_output_file)
    return results


def aggregate_scores_for_experiment(score_file, labels=None, metrics=Evaluator.default_metrics, nanmean=True, json_output_file=None,
                                    json_name="", json_description="", json_author="Fabian", json_task=""):
    """score_file: .npy of shape [cases, labels, metrics] -> the summary document (plain mean over the cases, as in the reference)"""
    scores = np.load(score_file)
    labels = [str(i) for i in range(scores.shape[1])] if labels is None else labels

    def table(block):
        return OrderedDict((label, OrderedDict((m, float(block[l][k])) for k, m in enumerate(metrics))) for l, label in enumerate(labels))
    doc = _summary(json_name, json_description, json_task, json_author, {"all": [table(case) for case in scores], "mean": table(scores.mean(0))})
    if json_output_file is not None:
        with open(json_output_file, "w") as f:
            json.dump(doc, f, indent=4, separators=(",", ": "))
    return doc


def evaluate_folder(folder_with_gts, folder_with_predictions, labels, **metric_kwargs):
    """Scores every .nii.gz of folder_with_predictions against the file of the same name in folder_with_gts (both folders must hold the same
    names) and writes folder_with_predictions/summary.json; surface metrics included, rv_rejection on, as in the fork (evaluator.py:486-487).
    surface= and surface_dice_threshold= reach Evaluator.evaluate."""
    files_gt = subfiles(folder_with_gts, suffix=".nii.gz", join_=False)
    files_pred = subfiles(folder_with_predictions, suffix=".nii.gz", join_=False)
    assert set(files_gt) <= set(files_pred), "files missing in folder_with_predictions"
    assert set(files_pred) <= set(files_gt), "files missing in folder_with_gts"
    pairs = [(join(folder_with_predictions, f), join(folder_with_gts, f)) for f in files_pred]
    return aggregate_scores(pairs, json_output_file=join(folder_with_predictions, "summary.json"), num_threads=8, labels=labels, advanced=True,
                            rv_rejection=True, **metric_kwargs)


# ------------------------------------------------------------------------------------------------ region-based evaluation
def get_brats_regions():
    """the BraTS regions on the labels 1, 2, 3 of the nnU-Net conversion (not the original BraTS convention)"""
    return {"whole tumor": (1, 2, 3), "tumor core": (2, 3), "enhancing tumor": (3,)}


def get_KiTS_regions():
    return {"kidney incl tumor": (1, 2), "tumor": (2,)}


def create_region_from_mask(mask, join_labels):
    """uint8 mask of the voxels of `mask` that hold one of `join_labels`"""
    return np.isin(np.asarray(mask), list(join_labels)).astype(np.uint8)


def _region_dice(hist, region):
    """hist[test label, reference label] -> Dice of the region (the union of its label values); NaN when it is empty in both"""
    idx = sorted(set(int(c) for c in region))
    n_pred, n_gt = int(hist[idx, :].sum()), int(hist[:, idx].sum())
    if n_pred == 0 and n_gt == 0:
        return float("nan")
    return 2.0 * int(hist[np.ix_(idx, idx)].sum()) / float(n_pred + n_gt)


def _label_histogram(pred, gt, what):
    """[K,K] counts of (pred label, gt label) with K = 1 + the largest label: cf_label_confusion on the device where both volumes hold
    labels below HIST_K (every nnU-Net label set in practice), numpy's bincount otherwise"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.shape != gt.shape:
        raise ValueError("%s: prediction %s and ground truth %s differ in shape" % (what, pred.shape, gt.shape))
    ev = Evaluator(pred, gt, labels=[])
    got = ev._histogram()
    if got is not None:
        return got[0]
    if pred.min() < 0 or gt.min() < 0 or np.any(pred != np.round(pred)) or np.any(gt != np.round(gt)):
        raise ValueError("%s: label volumes must hold non-negative integers" % what)
    p, g = pred.astype(np.int64).ravel(), gt.astype(np.int64).ravel()
    K = int(max(p.max(), g.max())) + 1
    return np.bincount(p * K + g, minlength=K * K).reshape(K, K)


def _score_regions(pred, gt, regions, what="case"):
    hist = _label_histogram(pred, gt, what)
    K = hist.shape[0]
    out = []
    for r in regions:
        inside = [c for c in r if 0 <= int(c) < K]                   # a label value beyond the histogram occurs in neither volume
        out.append(_region_dice(hist, inside) if inside else float("nan"))
    return out


def evaluate_case(file_pred, file_gt, regions):
    """Dice of every region (a list of label tuples) between two label files, NaN for a region empty in both; each file is read once"""
    return _score_regions(load_volume(file_pred).array, load_volume(file_gt).array, regions, file_pred)


def evaluate_regions(folder_predicted, folder_gt, regions, processes=8):
    """Scores every .nii.gz of folder_predicted against the file of the same name in folder_gt, region by region (regions: an ordered
    {name: labels}), and writes folder_predicted/summary.csv: one row per case, then mean, median (both ignoring NaN) and the two with NaN
    counted as 1, every number as "%02.4f".  A prediction without ground truth is an error, ground truth without a prediction a warning.
    processes: reader threads (files are read and inflated ahead of the device); only this process opens the GPU.
    Returns {region name: [Dice per case]}."""
    names = list(regions.keys())
    files_pred = subfiles(folder_predicted, suffix=".nii.gz", join_=False)
    files_gt = subfiles(folder_gt, suffix=".nii.gz", join_=False)
    assert all(f in files_gt for f in files_pred), "Some files in folder_predicted have not ground truth in folder_gt"
    if any(f not in files_pred for f in files_gt):
        print("WARNING! Some files in folder_gt were not predicted (not present in folder_predicted)!")
    files_pred.sort()
    region_labels = [tuple(v) for v in regions.values()]
    processes = max(1, int(processes))
    cases = read_ahead([(join(folder_predicted, f), join(folder_gt, f)) for f in files_pred], load_volume, depth=processes, readers=processes)
    res = [_score_regions(p.array, g.array, region_labels, f) for (_, (p, g)), f in zip(cases, files_pred)]
    scores = {r: [case[k] for case in res] for k, r in enumerate(names)}
    as_one = {r: np.where(np.isnan(v), 1.0, v) for r, v in ((r, np.asarray(scores[r], dtype=np.float64)) for r in names)}

    def row(title, values):
        return title + "".join(",%02.4f" % v for v in values) + "\n"

    with open(join(folder_predicted, "summary.csv"), "w") as f, warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # a region that is NaN in every case: nanmean of nothing is NaN
        f.write("casename" + "".join(",%s" % r for r in names) + "\n")
        for name, case in zip(files_pred, res):
            f.write(row(name[:-7], case))
        f.write(row("mean", [np.nanmean(scores[r]) for r in names]))
        f.write(row("median", [np.nanmedian(scores[r]) for r in names]))
        f.write(row("mean (nan is 1)", [np.mean(as_one[r]) for r in names]))
        f.write(row("median (nan is 1)", [np.median(as_one[r]) for r in names]))
    return scores


REGION_SETS = {"brats": get_brats_regions, "kits": get_KiTS_regions}


def parse_regions(spec):
    """--regions: 'brats', 'kits' or a JSON object {region name: [label values]} -> ordered {name: tuple of labels}"""
    if spec in REGION_SETS:
        return REGION_SETS[spec]()
    try:
        regions = json.loads(spec)
    except ValueError as e:
        raise ValueError("--regions %r is neither brats, kits nor a JSON object {region name: [labels]}: %s" % (spec, e))
    if not isinstance(regions, dict) or not regions or any(not isinstance(v, list) or not v for v in regions.values()):
        raise ValueError("--regions %r must be a non-empty JSON object {region name: non-empty list of labels}" % (spec,))
    return OrderedDict((str(k), tuple(int(c) for c in v)) for k, v in regions.items())


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Scores the label files of -pred against those of -ref and writes PRED/summary.json: the "
                                                 "scores of every case under 'all', their means over the cases under 'mean'.")
    parser.add_argument("-ref", required=True, type=str, help="folder of the reference label files (.nii.gz)")
    parser.add_argument("-pred", required=True, type=str, help="folder of the predicted label files, named like the reference ones")
    parser.add_argument("-l", nargs="+", type=int, default=None,
                        help="label values to score, e.g. -l 1 2 3 (0 is the background); required unless --regions is given")
    parser.add_argument("--regions", default=None, metavar="brats|kits|JSON",
                        help="region-based evaluation instead (-l is not read): Dice per region into PRED/summary.csv; brats, kits, or a JSON "
                             "object {region name: [labels]}")
    parser.add_argument("--surface", choices=("auto", "pairs", "edt"), default="auto",
                        help="how the surface metrics find their distances: pairs = all-pairs search (small objects), edt = exact distance "
                             "transform, one device visit per case (3-D organs), auto = pairs unless an object is large (default)")
    parser.add_argument("--surface_dice", type=float, default=None, metavar="MM",
                        help="also report the Normalized Surface Dice at this tolerance in mm")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.regions is not None:
        return evaluate_regions(args.pred, args.ref, parse_regions(args.regions))
    if args.l is None:
        parser.error("the following arguments are required: -l (or --regions)")
    extra = {} if args.surface_dice is None else {"surface_dice_threshold": args.surface_dice}
    return evaluate_folder(args.ref, args.pred, args.l, surface=args.surface, **extra)


nnunet_evaluate_folder = main

if __name__ == "__main__":
    main()
