"""Downstream metrics on the device: the functions the reference's compute_metrics*.py and
compute_jacobian.py apply to the Segmentation / Registered / Flow outputs of the path.

Mirrors nnunet/evaluation/metrics.py (ConfusionMatrix and the metric functions, same names, arguments and NaN rules) and the
per-frame statistics of nnunet/compute_jacobian.py.  numpy arrays or device tensors in, Python floats out like the reference.
Counting, border extraction, nearest-border distances and reductions are HIP kernels (csrc/metrics.hip); the 95th percentile of
hausdorff_distance_95 is taken by numpy on the downloaded distance vector (a few thousand values).
cine_label_scores / cine_jacobian_table (csrc/score.hip) give the same figures for all frames, classes and slices of a patient in one
device visit; cineflow.score writes the scripts' tables from them.  distance_transform_edt, surface_distances(method="edt"),
label_surface_edt_table and normalized_surface_dice (csrc/edt.hip) are the route for 3-D label volumes: scipy's exact Euclidean distance
transform on the device and medpy's surface distances read from it, all labels of a case in one visit, linear in the volume.
"""
import ctypes

import numpy as np
import torch

from . import ops
from ._lib import CineflowError, check, lib
from .ops import _f32, _stream, _u8


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _mask(a):
    """`a != 0` as a contiguous uint8 device tensor"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(_dev()) != 0).to(torch.uint8).contiguous()


def assert_shape(test, reference):
    assert test.shape == reference.shape, "Shape mismatch: {} and {}".format(test.shape, reference.shape)


class ConfusionMatrix:
    """metrics.py:27-105."""

    def __init__(self, test=None, reference=None):
        self.tp = self.fp = self.tn = self.fn = self.size = None
        self.reference_empty = self.reference_full = self.test_empty = self.test_full = None
        self.set_reference(reference)
        self.set_test(test)

    def set_test(self, test):
        self.test = test
        self.reset()

    def set_reference(self, reference):
        self.reference = reference
        self.reset()

    def reset(self):
        self.tp = self.fp = self.tn = self.fn = self.size = None
        self.test_empty = self.test_full = self.reference_empty = self.reference_full = None

    def compute(self):
        if self.test is None or self.reference is None:
            raise ValueError("'test' and 'reference' must both be set to compute confusion matrix.")
        assert_shape(self.test, self.reference)
        t, r = _mask(self.test), _mask(self.reference)
        n = t.numel()
        out = torch.empty(3, dtype=torch.int64, device=t.device)
        check(lib().cf_confusion_counts(_u8(t), _u8(r), n, out.data_ptr(), _stream()), "cf_confusion_counts")
        self.tp, self.fp, self.fn = (int(v) for v in out.cpu().tolist())
        self.tn = n - self.tp - self.fp - self.fn
        self.size = n
        self.test_empty, self.test_full = self.tp + self.fp == 0, self.tp + self.fp == n
        self.reference_empty, self.reference_full = self.tp + self.fn == 0, self.tp + self.fn == n

    def get_matrix(self):
        if None in (self.tp, self.fp, self.tn, self.fn):
            self.compute()
        return self.tp, self.fp, self.tn, self.fn

    def get_size(self):
        if self.size is None:
            self.compute()
        return self.size

    def get_existence(self):
        if None in (self.test_empty, self.test_full, self.reference_empty, self.reference_full):
            self.compute()
        return self.test_empty, self.test_full, self.reference_empty, self.reference_full


def _nan(nan_for_nonexisting):
    return float("NaN") if nan_for_nonexisting else 0.


def _cm(test, reference, confusion_matrix):
    return ConfusionMatrix(test, reference) if confusion_matrix is None else confusion_matrix


def dice(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """2TP / (2TP + FP + FN)  (metrics.py:107-129)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    test_empty, test_full, reference_empty, reference_full = cm.get_existence()
    if test_empty and reference_empty:
        return _nan(nan_for_nonexisting)
    return float(2. * tp / (2 * tp + fp + fn))


def jaccard(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TP / (TP + FP + FN)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    test_empty, test_full, reference_empty, reference_full = cm.get_existence()
    if test_empty and reference_empty:
        return _nan(nan_for_nonexisting)
    return float(tp / (tp + fp + fn))


def precision(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TP / (TP + FP)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    if cm.get_existence()[0]:
        return _nan(nan_for_nonexisting)
    return float(tp / (tp + fp))


def sensitivity(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TP / (TP + FN)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    if cm.get_existence()[2]:
        return _nan(nan_for_nonexisting)
    return float(tp / (tp + fn))


def recall(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TP / (TP + FN)"""
    return sensitivity(test, reference, confusion_matrix, nan_for_nonexisting, **kwargs)


def specificity(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TN / (TN + FP)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    if cm.get_existence()[3]:
        return _nan(nan_for_nonexisting)
    return float(tn / (tn + fp))


def accuracy(test=None, reference=None, confusion_matrix=None, **kwargs):
    """(TP + TN) / (TP + FP + FN + TN)"""
    tp, fp, tn, fn = _cm(test, reference, confusion_matrix).get_matrix()
    return float((tp + tn) / (tp + fp + tn + fn))


def fscore(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, beta=1., **kwargs):
    """(1 + b^2) * TP / ((1 + b^2) * TP + b^2 * FN + FP)"""
    precision_ = precision(test, reference, confusion_matrix, nan_for_nonexisting)
    recall_ = recall(test, reference, confusion_matrix, nan_for_nonexisting)
    return (1 + beta * beta) * precision_ * recall_ / ((beta * beta * precision_) + recall_)


def false_positive_rate(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """FP / (FP + TN)"""
    return 1 - specificity(test, reference, confusion_matrix, nan_for_nonexisting)


def false_omission_rate(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """FN / (TN + FN)"""
    cm = _cm(test, reference, confusion_matrix)
    tp, fp, tn, fn = cm.get_matrix()
    if cm.get_existence()[1]:
        return _nan(nan_for_nonexisting)
    return float(fn / (fn + tn))


def false_negative_rate(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """FN / (TP + FN)"""
    return 1 - sensitivity(test, reference, confusion_matrix, nan_for_nonexisting)


def true_negative_rate(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TN / (TN + FP)"""
    return specificity(test, reference, confusion_matrix, nan_for_nonexisting)


def false_discovery_rate(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """FP / (TP + FP)"""
    return 1 - precision(test, reference, confusion_matrix, nan_for_nonexisting)


def negative_predictive_value(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, **kwargs):
    """TN / (TN + FN)"""
    return 1 - false_omission_rate(test, reference, confusion_matrix, nan_for_nonexisting)


def total_positives_test(test=None, reference=None, confusion_matrix=None, **kwargs):
    """TP + FP"""
    tp, fp, tn, fn = _cm(test, reference, confusion_matrix).get_matrix()
    return tp + fp


def total_negatives_test(test=None, reference=None, confusion_matrix=None, **kwargs):
    """TN + FN"""
    tp, fp, tn, fn = _cm(test, reference, confusion_matrix).get_matrix()
    return tn + fn


def total_positives_reference(test=None, reference=None, confusion_matrix=None, **kwargs):
    """TP + FN"""
    tp, fp, tn, fn = _cm(test, reference, confusion_matrix).get_matrix()
    return tp + fn


def total_negatives_reference(test=None, reference=None, confusion_matrix=None, **kwargs):
    """TN + FP"""
    tp, fp, tn, fn = _cm(test, reference, confusion_matrix).get_matrix()
    return tn + fp


# ------------------------------------------------------------------------------------------------ surface distances
def _border(mask):
    shape = tuple(mask.shape)
    assert len(shape) in (2, 3), "surface distances are built for 2-D and 3-D masks"
    D, H, W = (1,) * (3 - len(shape)) + shape
    coords = torch.empty(3 * mask.numel(), dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int32, device=mask.device)
    check(lib().cf_surface_border(_u8(mask), D, H, W, len(shape), coords.data_ptr(), count.data_ptr(), _stream()), "cf_surface_border")
    return coords, int(count.item())


# `auto` (method=None) leaves the all-pairs search for the transform when na x nb -- the border voxels of the two masks -- exceeds this.
# profiles/edt_table.md: on two offset balls the transform won every repeat from na x nb = 6.6e6 on (2^23), but the suite's own masks reach
# 4999 x 4999 on the default route (tests/test_gpu_metrics_kernels.py), and no input an existing test uses may change route: 2^25.
EDT_AUTO_PAIRS = 1 << 25
SURFACE_METHODS = (None, "pairs", "edt")


def _no_cpu_tensor(a, name):
    if torch.is_tensor(a) and not a.is_cuda:
        raise TypeError("%s must be a CUDA/HIP tensor or a numpy array (cineflow has no CPU path)" % name)


def _spacing3(spacing, nd):
    sp = np.ones(nd) if spacing is None else np.asarray(spacing, dtype=np.float64) * np.ones(nd)
    return [1.0] * (3 - nd) + [float(v) for v in sp]


def _edt_workspace(D, H, W, device):
    size = lib().cf_edt_workspace_bytes(D, H, W)
    if size < 0:
        check(int(size), "cf_edt_workspace_bytes")
    return torch.empty(int(size), dtype=torch.uint8, device=device)


def distance_transform_edt(input, sampling=None, return_distances=True, return_indices=False, distances=None, indices=None):
    """scipy.ndimage.distance_transform_edt for 2-D and 3-D inputs: the distance of every element to the nearest element that is 0, with
    `sampling` the spacing along each axis (a number or one per axis) -> fp64 device tensor of input's shape, scipy's bits whenever the
    squared terms are exact in fp64 (cf_edt).  Only the distances are built: return_distances=False, return_indices, distances= and
    indices= raise NotImplementedError.  An input without any zero raises (scipy's result there is meaningless)."""
    for name, given in (("return_distances", return_distances is not True), ("return_indices", bool(return_indices)),
                        ("distances", distances is not None), ("indices", indices is not None)):
        if given:
            raise NotImplementedError("distance_transform_edt: %s is not built (only the distance map is returned)" % name)
    _no_cpu_tensor(input, "input")
    m = _mask(input)
    nd = m.dim()
    if nd not in (2, 3):
        raise NotImplementedError("distance_transform_edt is built for 2-D and 3-D inputs, got %d-D" % nd)
    D, H, W = (1,) * (3 - nd) + tuple(m.shape)
    sz, sy, sx = _spacing3(sampling, nd)
    ws = _edt_workspace(D, H, W, m.device)
    out = torch.empty(tuple(m.shape), dtype=torch.float64, device=m.device)
    check(lib().cf_edt(_u8(m), D, H, W, nd, sz, sy, sx, ws.data_ptr(), out.data_ptr(), _stream()), "cf_edt")
    if int(ws[24:28].view(torch.int32).item()):                  # the library never synchronises: "no zero anywhere" comes back as a status word
        raise CineflowError("cf_edt failed (-1): the input holds no zero element, so no distance is defined")
    return out


def _label_surface_edt(t, r, labels, voxel_spacing, capacity=None, score_full=False):
    """one cf_label_surface_edt call on uint8 device volumes -> (head row table [K, 8] and offsets [2 K + 1] on the host, dist on the device)"""
    assert_shape(t, r)
    nd = t.dim()
    assert nd in (2, 3), "surface distances are built for 2-D and 3-D volumes"
    D, H, W = (1,) * (3 - nd) + tuple(t.shape)
    sz, sy, sx = _spacing3(voxel_spacing, nd)
    labs = [int(l) for l in labels]
    K = len(labs)
    n = t.numel()
    cap = max(1, 2 * n if capacity is None else min(2 * n, int(capacity)))
    ws = _edt_workspace(D, H, W, t.device)
    dist = torch.empty(cap, dtype=torch.float64, device=t.device)
    head = torch.empty(10 * K + 2, dtype=torch.float64, device=t.device)
    check(lib().cf_label_surface_edt(_u8(t), _u8(r), D, H, W, nd, (ctypes.c_int * K)(*labs), K, sz, sy, sx, int(bool(score_full)), ws.data_ptr(),
                                     dist.data_ptr(), cap, head.data_ptr(), _stream()), "cf_label_surface_edt")
    hd = head.cpu().numpy()
    if hd[-1]:
        raise CineflowError("cf_label_surface_edt: the distances did not fit the buffer of %d values" % cap)
    return hd[2 * K + 1:-1].reshape(K, 8), hd[:2 * K + 1].astype(np.int64), dist


def _surface_distances_edt(a, b, voxelspacing):
    rows, offs, dist = _label_surface_edt(a, b, [1], voxelspacing, score_full=True)
    if rows[0, 6] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if rows[0, 7] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return dist[offs[0]:offs[1]].clone()


def surface_distances(result, reference, voxelspacing=None, connectivity=1, method=None):
    """medpy.metric.binary.__surface_distances: distance of every border voxel of `result` to the nearest border voxel of
    `reference` -> fp64 device tensor.  method "pairs": the all-pairs search (values in no particular order); "edt": read from the exact
    distance transform of reference's border (cf_label_surface_edt; values in raster order of result's border voxels, the same on every
    run); None: "pairs" unless the two borders hold more than EDT_AUTO_PAIRS pairs."""
    if method not in SURFACE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (SURFACE_METHODS, method))
    if connectivity != 1:
        raise NotImplementedError("surface distances are built for connectivity 1 (the reference's only value)")
    if method == "edt":
        _no_cpu_tensor(result, "result")
        _no_cpu_tensor(reference, "reference")
    a, b = _mask(result), _mask(reference)
    assert_shape(a, b)
    if method == "edt":
        return _surface_distances_edt(a, b, voxelspacing)
    nd = a.dim()
    sz, sy, sx = _spacing3(voxelspacing, nd)
    ca, na = _border(a)
    cb, nb = _border(b)
    if na == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if nb == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    if method is None and na * nb > EDT_AUTO_PAIRS:
        return _surface_distances_edt(a, b, voxelspacing)
    dist = torch.empty(na, dtype=torch.float64, device=a.device)
    check(lib().cf_surface_min_dist(ca.data_ptr(), na, cb.data_ptr(), nb, sz, sy, sx, dist.data_ptr(), _stream()), "cf_surface_min_dist")
    return dist


def surface_dice_from_distances(a_to_b, b_to_a, threshold):
    """the arithmetic of nnunet/evaluation/surface_dice.py:46-56 on the two directed distance vectors (host arrays): the share of each
    surface within `threshold` (<=) against the share beyond it (>), with the 1e-8 that keeps the quotient defined"""
    a_to_b, b_to_a = np.asarray(a_to_b), np.asarray(b_to_a)
    numel_a, numel_b = len(a_to_b), len(b_to_a)
    tp_a = np.sum(a_to_b <= threshold) / numel_a
    tp_b = np.sum(b_to_a <= threshold) / numel_b
    fp = np.sum(a_to_b > threshold) / numel_a
    fn = np.sum(b_to_a > threshold) / numel_b
    return float((tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8))


def normalized_surface_dice(a, b, threshold, spacing=None, connectivity=1, method=None):
    """nnunet/evaluation/surface_dice.py:20-56 (not the official surface Dice, as the reference says itself): symmetric, threshold in mm"""
    _no_cpu_tensor(a, "a")
    _no_cpu_tensor(b, "b")
    assert tuple(np.shape(a)) == tuple(np.shape(b)), "a and b must have the same shape. a.shape= %s, b.shape= %s" % (np.shape(a), np.shape(b))
    a_to_b = surface_distances(a, b, spacing, connectivity, method)
    b_to_a = surface_distances(b, a, spacing, connectivity, method)
    return surface_dice_from_distances(a_to_b.cpu().numpy(), b_to_a.cpu().numpy(), threshold)


def _max_sum(dist):
    out = torch.empty(2, dtype=torch.float64, device=dist.device)
    check(lib().cf_max_sum_nonneg(dist.data_ptr(), dist.numel(), out.data_ptr(), _stream()), "cf_max_sum_nonneg")
    mx, sm = out.cpu().tolist()
    return mx, sm


def _mean_distance(dist, reproducible):
    """mean of a distance vector.  The vector's order follows the border compaction (one atomic per wave), so the device sum rounds
    differently from call to call; reproducible=True sums the sorted vector on the host instead: one value for one pair of masks."""
    if reproducible:
        return float(np.sum(np.sort(dist.cpu().numpy())) / dist.numel())
    return _max_sum(dist)[1] / dist.numel()


def _surface_metric(kind, test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, reproducible=False, method=None,
                    threshold=None):
    cm = _cm(test, reference, confusion_matrix)
    test_empty, test_full, reference_empty, reference_full = cm.get_existence()
    if test_empty or test_full or reference_empty or reference_full:
        return float("NaN") if nan_for_nonexisting else 0
    test, reference = cm.test, cm.reference
    d1 = surface_distances(test, reference, voxel_spacing, connectivity, method)
    if kind == "asd":
        return _mean_distance(d1, reproducible)
    d2 = surface_distances(reference, test, voxel_spacing, connectivity, method)
    if kind == "nsd":
        return surface_dice_from_distances(d1.cpu().numpy(), d2.cpu().numpy(), threshold)
    if kind == "hd":
        return max(_max_sum(d1)[0], _max_sum(d2)[0])
    if kind == "assd":
        return float(np.mean((_mean_distance(d1, reproducible), _mean_distance(d2, reproducible))))
    return float(np.percentile(np.hstack((d1.cpu().numpy(), d2.cpu().numpy())), 95))


def hausdorff_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1, method=None,
                       **kwargs):
    """metrics.py:323-338 (medpy.metric.hd)."""
    return _surface_metric("hd", test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, method=method)


def hausdorff_distance_95(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1, method=None,
                          **kwargs):
    """metrics.py:341-356 (medpy.metric.hd95)."""
    return _surface_metric("hd95", test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, method=method)


def avg_surface_distance(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1,
                         reproducible=False, method=None, **kwargs):
    """metrics.py:359-374 (medpy.metric.asd)."""
    return _surface_metric("asd", test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, reproducible, method)


def avg_surface_distance_symmetric(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1,
                                   reproducible=False, method=None, **kwargs):
    """metrics.py:377-392 (medpy.metric.assd)."""
    return _surface_metric("assd", test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, reproducible, method)


def normalized_surface_dice_metric(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1,
                                   threshold=1.0, method=None, **kwargs):
    """normalized_surface_dice under the existence rules of the other surface metrics (NaN where a mask is empty or fills the volume)"""
    return _surface_metric("nsd", test, reference, confusion_matrix, nan_for_nonexisting, voxel_spacing, connectivity, method=method, threshold=threshold)


ALL_METRICS = {
    "False Positive Rate": false_positive_rate, "Dice": dice, "Jaccard": jaccard, "Hausdorff Distance": hausdorff_distance,
    "Hausdorff Distance 95": hausdorff_distance_95, "Precision": precision, "Recall": recall,
    "Avg. Symmetric Surface Distance": avg_surface_distance_symmetric, "Avg. Surface Distance": avg_surface_distance, "Accuracy": accuracy,
    "False Omission Rate": false_omission_rate, "Negative Predictive Value": negative_predictive_value,
    "False Negative Rate": false_negative_rate, "True Negative Rate": true_negative_rate, "False Discovery Rate": false_discovery_rate,
    "Total Positives Test": total_positives_test, "Total Negatives Test": total_negatives_test,
    "Total Positives Reference": total_positives_reference, "total Negatives Reference": total_negatives_reference,
}


def label_volume_u8(a, what="label volume"):
    """numpy array or tensor holding the integers 0..255 (in any integer or float dtype) -> contiguous uint8 device tensor; anything else
    is refused (_cast_labels_u8 is the cast that does not look)"""
    if torch.is_tensor(a):
        a = a.cpu().numpy() if a.dtype != torch.uint8 else a
    if torch.is_tensor(a):
        return a.to(_dev()).contiguous()
    a = np.asarray(a)
    if a.dtype != np.uint8:
        as_u8 = a.astype(np.uint8) if a.size and a.min() >= 0 and a.max() <= 255 else None
        if as_u8 is None or not np.array_equal(as_u8, a):
            raise ValueError("%s: the values must be the integers 0..255 (dtype %s, range %s..%s)"
                             % (what, a.dtype, a.min() if a.size else "-", a.max() if a.size else "-"))
        a = as_u8
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _cast_labels_u8(a):
    """label volume -> contiguous uint8 device tensor by a plain cast, no value check (label_volume_u8 is the one that refuses)"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(_dev()).to(torch.uint8).contiguous()


def label_histogram(t, r, K):
    """One cf_label_confusion launch on two uint8 device tensors of one shape -> (hist [K,K] int64 numpy of counts[t label, r label], the
    number of voxels with a label >= K in either volume, which are in no cell)"""
    assert_shape(t, r)
    hist = torch.empty(K * K + 1, dtype=torch.int64, device=t.device)
    check(lib().cf_label_confusion(_u8(t), _u8(r), t.numel(), K, hist.data_ptr(), _stream()), "cf_label_confusion")
    h = hist.cpu().numpy()
    return h[:-1].reshape(K, K), int(h[-1])


def label_confusion(test, reference, num_classes):
    """All classes of nnunet/compute_metrics.py:96-106 in one pass: K x K int64 matrix M[t, r] = #voxels with test label t and
    reference label r (labels must be < num_classes <= 16); per-class Dice = 2 M[c,c] / (M[c,:].sum() + M[:,c].sum())."""
    K = int(num_classes)
    hist, overflow = label_histogram(_cast_labels_u8(test), _cast_labels_u8(reference), K)
    if overflow:
        raise ValueError("label_confusion: %d voxels carry a label >= num_classes=%d" % (overflow, K))
    return hist


# ------------------------------------------------------------------------------------------------ compute_jacobian.py
def jacobian_determinant(disp):
    """compute_jacobian.py:16-60 for a 2-D displacement field [H, W, 2] (channel-last like the script) -> float64 [H, W] (numpy for a
    numpy field, device tensor for a tensor)."""
    was_numpy = not torch.is_tensor(disp)
    d = torch.from_numpy(np.ascontiguousarray(disp)) if was_numpy else disp
    assert d.dim() == 3 and d.shape[-1] == 2, "flow has to be [H, W, 2]"
    flow = d.to(_dev(), dtype=torch.float32).permute(2, 0, 1)[None].contiguous()
    jac = ops.jacobian_det(flow)[0]
    return jac.cpu().numpy() if was_numpy else jac


def jacobian_frame_stats(frame_flow, frame_gt, names=("RV", "MYO", "LV")):
    """compute_jacobian.py:151-186: the per-frame row of the Jacobian table (structures = labels 1..len(names) of frame_gt)."""
    jac = jacobian_determinant(frame_flow)
    jac_t = jac if torch.is_tensor(jac) else torch.from_numpy(np.ascontiguousarray(jac))
    jac_t = jac_t.to(_dev(), dtype=torch.float64).contiguous()
    gt = (frame_gt if torch.is_tensor(frame_gt) else torch.from_numpy(np.ascontiguousarray(frame_gt))).to(_dev())
    K = len(names) + 1
    lab = torch.where((gt >= 0) & (gt < K), gt, torch.full_like(gt, 255)).to(torch.uint8).contiguous()
    stats = torch.empty(3 * K, dtype=torch.float64, device=lab.device)
    check(lib().cf_region_stats(jac_t.data_ptr(), _u8(lab), lab.numel(), K, stats.data_ptr(), _stream()), "cf_region_stats")
    whole = torch.empty(3, dtype=torch.float64, device=lab.device)
    zeros = torch.zeros_like(lab)
    check(lib().cf_region_stats(jac_t.data_ptr(), _u8(zeros), lab.numel(), 1, whole.data_ptr(), _stream()), "cf_region_stats")
    st = stats.cpu().numpy().reshape(K, 3)
    res = {}
    for i, k in enumerate(names, 1):
        s, total, neg = st[i]
        res["abs(Mean jacobian - 1)_" + k] = abs(s / total - 1) if total else float("nan")
        res["total_" + k] = float(total)
        res["negative_" + k] = float(neg)
        res["negative_%_" + k] = (neg / total) * 100 if total else float("nan")
    res["abs(Mean jacobian - 1)_average"] = sum(res["abs(Mean jacobian - 1)_" + k] for k in names) / 3
    res["negative_%_average"] = sum(res["negative_%_" + k] for k in names) / 3
    s, total, neg = whole.cpu().tolist()
    res["abs(Mean jacobian - 1)"] = abs(s / total - 1)
    res["total"] = float(total)
    res["negative"] = float(neg)
    res["negative_%"] = (neg / total) * 100
    return res


def spatial_gradient3d(x):
    """kornia.filters.spatial_gradient3d(x, mode='diff', order=1): [B, C, D, H, W] fp32 -> [B, C, 3, D, H, W]."""
    was_numpy = not torch.is_tensor(x)
    t = (torch.from_numpy(np.ascontiguousarray(x)) if was_numpy else x).to(_dev(), dtype=torch.float32).contiguous()
    B, C, D, H, W = t.shape
    out = torch.empty((B, C, 3, D, H, W), dtype=torch.float32, device=t.device)
    check(lib().cf_spatial_gradient3d(_f32(t), _f32(out), B * C, D, H, W, _stream()), "cf_spatial_gradient3d")
    return out.cpu().numpy() if was_numpy else out


def gradient_means(slice_flow):
    """compute_jacobian.py:146-159: slice_flow [T, H, W, 2] -> (temporal gradient [T], spatial gradient [T]): the per-frame means
    of |d/dt| and of |d/dx|, |d/dy| of both flow components."""
    t = (slice_flow if torch.is_tensor(slice_flow) else torch.from_numpy(np.ascontiguousarray(slice_flow))).to(_dev(), dtype=torch.float32)
    T, H, W, _ = t.shape
    g = spatial_gradient3d(t.permute(3, 0, 1, 2)[None].contiguous())          # [1, 2, 3, T, H, W]
    sums = torch.empty(2 * 3 * T, dtype=torch.float64, device=g.device)         # slabs (c, comp) x frame
    check(lib().cf_slab_abs_sum(_f32(g), 6, 1, T, H * W, sums.data_ptr(), _stream()), "cf_slab_abs_sum")
    s = sums.cpu().numpy().reshape(2, 3, T)
    return s[:, 2].sum(0) / (2 * H * W), s[:, :2].sum((0, 1)) / (4 * H * W)


# ------------------------------------------------------------------------------------------------ one visit per patient
def label_surface_table(test, reference, num_classes, voxel_spacing=None):
    """All frames and classes of a patient in two library calls (cf_label_surface_count, cf_label_surface_table) and three reads.

    test / reference: label stacks [N, H, W] (2-D frames) or [N, D, H, W] (3-D frames), labels < num_classes <= 16.  Returns
    (table, dist, offsets): table float64 [N, K, 9] = {TP, FP, FN, border voxels of test, of reference, max test->ref, max ref->test,
    sum test->ref, sum ref->test} of `test == c` vs `reference == c` (row 0, the background, is not scored and stays zero); dist the
    directed nearest-border distances of every border voxel; offsets int [N, K, 2, 2]: the distances of (n, c, side) -- side 0 test->ref,
    1 ref->test -- are dist[offsets[n, c, side, 0]:offsets[n, c, side, 1]], in compaction order.  Where one side of a pair has no border the
    other side's distances are not computed (NaN).  The distance search is brute force: cine-sized objects, not hundreds of thousands of
    border voxels."""
    t, r = _cast_labels_u8(test), _cast_labels_u8(reference)
    assert_shape(t, r)
    assert t.dim() in (3, 4), "label stacks are [N, H, W] or [N, D, H, W]"
    nd = t.dim() - 1
    N = t.shape[0]
    D, H, W = (1,) * (3 - nd) + tuple(t.shape[1:])
    K = int(num_classes)
    sp = np.ones(nd) if voxel_spacing is None else np.asarray(voxel_spacing, dtype=np.float64) * np.ones(nd)
    sz, sy, sx = ([1.0] * (3 - nd) + [float(v) for v in sp])
    ws = torch.empty(11 * N * K + 3, dtype=torch.int32, device=t.device)
    table = torch.empty(9 * N * K + 1, dtype=torch.float64, device=t.device)
    check(lib().cf_label_surface_count(_u8(t), _u8(r), N, D, H, W, nd, K, ws.data_ptr(), table.data_ptr(), _stream()), "cf_label_surface_count")
    S = 2 * N * K
    scans = ws[5 * N * K + 1:5 * N * K + 1 + 2 * (S + 1)].cpu().numpy()
    offs, blk = scans[:S + 1].astype(np.int64), scans[S + 1:]
    total, nblocks = int(offs[S]), int(blk[S])
    coords = torch.empty(3 * max(total, 1), dtype=torch.int32, device=t.device)
    dist = torch.full((max(total, 1),), float("nan"), dtype=torch.float64, device=t.device)
    check(lib().cf_label_surface_table(_u8(t), _u8(r), N, D, H, W, nd, K, sz, sy, sx, ws.data_ptr(), total, nblocks, coords.data_ptr(), dist.data_ptr(),
                                       table.data_ptr(), _stream()), "cf_label_surface_table")
    tab = table.cpu().numpy()
    if tab[-1]:
        raise ValueError("label_surface_table: %d voxels carry a label >= num_classes=%d" % (int(tab[-1]), K))
    d = dist.cpu().numpy()[:total]
    return tab[:-1].reshape(N, K, 9), d, np.stack([offs[:-1], offs[1:]], -1).reshape(N, K, 2, 2)


def cine_label_scores(test, reference, num_classes, voxel_spacing=None, reproducible=True):
    """Dice, Hausdorff distance and surface distances of every frame and class of a patient from one label_surface_table visit: what
    nnunet/compute_metrics.py:96-106 asks of dice / hausdorff_distance / avg_surface_distance_symmetric frame by frame and class by class.

    Returns a dict of float64 arrays [N, K]: dice, hd, asd_test_to_ref, asd_ref_to_test, assd, hd95 (column 0, the background, is NaN).
    The existence rules are those of `dice` and `_surface_metric`: Dice is NaN when both masks are empty, the surface metrics when a mask
    is empty or fills the frame.  reproducible=True takes the means from each segment's distances sorted on the host (the rule of
    _mean_distance), so a value does not depend on the order of the border compaction; False divides the device sums.  Brute-force
    distance search: cine-sized objects only."""
    tab, dist, offs = label_surface_table(test, reference, num_classes, voxel_spacing)
    N, K = tab.shape[:2]
    V = int(np.prod(np.shape(test)[1:]))
    out = {k: np.full((N, K), np.nan) for k in ("dice", "hd", "asd_test_to_ref", "asd_ref_to_test", "assd", "hd95")}
    for n in range(N):
        for c in range(1, K):
            tp, fp, fn = (int(v) for v in tab[n, c, :3])
            nt, nr = tp + fp, tp + fn
            if nt or nr:
                out["dice"][n, c] = float(2. * tp / (2 * tp + fp + fn))
            if nt in (0, V) or nr in (0, V):
                continue
            d1, d2 = (dist[offs[n, c, s, 0]:offs[n, c, s, 1]] for s in (0, 1))
            if reproducible:
                m1, m2 = float(np.sum(np.sort(d1)) / d1.size), float(np.sum(np.sort(d2)) / d2.size)
            else:
                m1, m2 = float(tab[n, c, 7] / d1.size), float(tab[n, c, 8] / d2.size)
            out["hd"][n, c] = max(float(tab[n, c, 5]), float(tab[n, c, 6]))
            out["asd_test_to_ref"][n, c], out["asd_ref_to_test"][n, c] = m1, m2
            out["assd"][n, c] = float(np.mean((m1, m2)))
            out["hd95"][n, c] = float(np.percentile(np.hstack((d1, d2)), 95))
    return out


def label_surface_edt_table(test, reference, labels, voxel_spacing=None, capacity=None):
    """The surface metrics of every listed label of two 2-D or 3-D label volumes from ONE cf_label_surface_edt call: for label c the masks are
    `test == c` and `reference == c`, the distances come from the exact distance transform of the other mask's border inside the joint
    bounding box of the two borders, and nothing is searched over pairs.  Two reads: the offsets and the per-label table, then exactly
    the distances.  `labels`: up to 16 values 0..255.  capacity: an upper bound of the number of distances when the caller knows a
    better one than 2 x voxels (the voxels of the listed labels in both volumes, say).

    Returns {label: dict} with d_test_to_ref / d_ref_to_test (fp64 numpy, raster order of the border voxels they belong to), n_test /
    n_ref (border voxels), hd, hd95 (np.percentile of both vectors, 95), asd_test_to_ref, asd_ref_to_test (device sum / count: the
    order is fixed, so the value is the same on every run) and assd.  A label that has no voxel, or fills the volume, in either input
    gets empty vectors and NaN, the rule of hausdorff_distance and the others."""
    _no_cpu_tensor(test, "test")
    _no_cpu_tensor(reference, "reference")
    labs = [int(l) for l in labels]
    if not 1 <= len(labs) <= 16 or any(l < 0 or l > 255 for l in labs):
        raise ValueError("labels must be 1..16 values in 0..255, got %r" % (labs,))
    t, r = _cast_labels_u8(test), _cast_labels_u8(reference)
    rows, offs, dist = _label_surface_edt(t, r, labs, voxel_spacing, capacity)
    d = dist[:int(offs[-1])].cpu().numpy() if offs[-1] else np.zeros(0)
    out = {}
    nan = float("nan")
    for k, c in enumerate(labs):
        d1, d2 = d[offs[2 * k]:offs[2 * k + 1]], d[offs[2 * k + 1]:offs[2 * k + 2]]
        n1, n2 = int(rows[k, 0]), int(rows[k, 1])
        res = {"d_test_to_ref": d1, "d_ref_to_test": d2, "n_test": int(rows[k, 6]), "n_ref": int(rows[k, 7])}
        if n1 and n2:
            m1, m2 = float(rows[k, 4] / n1), float(rows[k, 5] / n2)
            res.update(hd=max(float(rows[k, 2]), float(rows[k, 3])), hd95=float(np.percentile(np.hstack((d1, d2)), 95)),
                       asd_test_to_ref=m1, asd_ref_to_test=m2, assd=float(np.mean((m1, m2))))
        else:
            res.update(hd=nan, hd95=nan, asd_test_to_ref=nan, asd_ref_to_test=nan, assd=nan)
        out[c] = res
    return out


def flow_regularity_table(flow, labels, num_classes):
    """cf_flow_regularity_table: flow [T, H, W, D, 2] (the stacked `flow` arrays of a patient's .npz files), labels [T, H, W, D] ->
    float64 [T, D, 5 + 3 K]: {sum |d/dt|, sum |d/dy| + |d/dx|} of both components, then {sum J, count, #(J < 0)} per label k < K and for
    the whole slice.  One call and one read; the same bits on every run."""
    f = (flow if torch.is_tensor(flow) else torch.from_numpy(np.ascontiguousarray(flow))).to(_dev(), dtype=torch.float32)
    assert f.dim() == 5 and f.shape[-1] == 2, "flow has to be [T, H, W, D, 2]"
    T, H, W, D, _ = f.shape
    g = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    assert tuple(g.shape) == (T, H, W, D), "Shape mismatch: flow {} and labels {}".format(tuple(f.shape), tuple(g.shape))
    g = g.to(_dev())
    K = int(num_classes)
    if g.dtype != torch.uint8:
        g = torch.where((g >= 0) & (g < K), g, torch.full_like(g, 255)).to(torch.uint8)
    f = f.permute(0, 3, 4, 1, 2).contiguous()                                   # [T, D, 2, H, W]
    g = g.permute(0, 3, 1, 2).contiguous()                                      # [T, D, H, W]
    cols = 5 + 3 * K
    part = torch.empty(T * D * (-(-H // 32)) * (-(-W // 64)) * cols, dtype=torch.float64, device=f.device)
    table = torch.empty(T * D * cols, dtype=torch.float64, device=f.device)
    check(lib().cf_flow_regularity_table(_f32(f), _u8(g), T, D, H, W, K, part.data_ptr(), table.data_ptr(), _stream()), "cf_flow_regularity_table")
    return table.cpu().numpy().reshape(T, D, cols)


def cine_jacobian_table(flow, labels, names=("RV", "MYO", "LV")):
    """compute_jacobian.py:141-198 for one patient: flow [T, H, W, D, 2], labels [T, H, W, D] (structures = labels 1..len(names)) -> one
    dict per (slice, frame), slices outermost like the script, holding `Temporal gradient`, `Spatial gradient` (gradient_means) and the
    keys of jacobian_frame_stats."""
    K = len(names) + 1
    tab = flow_regularity_table(flow, labels, K)
    T, D = tab.shape[:2]
    H, W = int(np.shape(flow)[1]), int(np.shape(flow)[2])
    rows = []
    for d in range(D):
        for t in range(T):
            v = tab[t, d]
            res = {"Temporal gradient": float(v[0] / (2 * H * W)), "Spatial gradient": float(v[1] / (4 * H * W))}
            for i, k in enumerate(names, 1):
                s, total, neg = v[2 + 3 * i:5 + 3 * i]
                res["abs(Mean jacobian - 1)_" + k] = float(abs(s / total - 1)) if total else float("nan")
                res["total_" + k] = float(total)
                res["negative_" + k] = float(neg)
                res["negative_%_" + k] = float((neg / total) * 100) if total else float("nan")
            res["abs(Mean jacobian - 1)_average"] = sum(res["abs(Mean jacobian - 1)_" + k] for k in names) / 3
            res["negative_%_average"] = sum(res["negative_%_" + k] for k in names) / 3
            s, total, neg = v[2 + 3 * K:5 + 3 * K]
            res["abs(Mean jacobian - 1)"] = float(abs(s / total - 1))
            res["total"] = float(total)
            res["negative"] = float(neg)
            res["negative_%"] = float((neg / total) * 100)
            rows.append(res)
    return rows


# ------------------------------------------------------------------------------------------------ compute_SSIM*.py
def structural_similarity(im1, im2, *, win_size=None, data_range=None, full=False, K1=0.01, K2=0.03, use_sample_covariance=True):
    """skimage.metrics.structural_similarity as nnunet/compute_SSIM.py:91 and compute_SSIM_crop_per_structure.py:88 call it: 2-D
    images, uniform win_size x win_size window (default 7), `data_range` given.  Computed in fp64 (skimage keeps float32 inputs in
    float32).  Returns the mean SSIM over the interior (the map cropped by (win_size - 1) // 2), and with full=True also the map."""
    a = (im1 if torch.is_tensor(im1) else torch.from_numpy(np.ascontiguousarray(im1))).to(_dev(), dtype=torch.float64).contiguous()
    b = (im2 if torch.is_tensor(im2) else torch.from_numpy(np.ascontiguousarray(im2))).to(_dev(), dtype=torch.float64).contiguous()
    assert_shape(a, b)
    if a.dim() != 2:
        raise NotImplementedError("structural_similarity is built for 2-D images (the reference scores slice by slice)")
    if data_range is None:
        raise ValueError("data_range must be given for floating-point images (as skimage requires)")
    win = 7 if win_size is None else int(win_size)
    H, W = a.shape
    if win % 2 == 0 or win > min(H, W):
        raise ValueError("win_size must be odd and no larger than the image")
    NP = win * win
    cov_norm = NP / (NP - 1.0) if use_sample_covariance else 1.0
    R = float(data_range)
    S = torch.empty((H, W), dtype=torch.float64, device=a.device)
    check(lib().cf_ssim_map(a.data_ptr(), b.data_ptr(), H, W, win, (K1 * R) ** 2, (K2 * R) ** 2, cov_norm, S.data_ptr(), _stream()), "cf_ssim_map")
    pad = (win - 1) // 2
    inner = S[pad:H - pad, pad:W - pad].contiguous()
    zeros = torch.zeros(inner.numel(), dtype=torch.uint8, device=a.device)
    st = torch.empty(3, dtype=torch.float64, device=a.device)
    check(lib().cf_region_stats(inner.data_ptr(), _u8(zeros), inner.numel(), 1, st.data_ptr(), _stream()), "cf_region_stats")
    s, cnt, _ = st.cpu().tolist()
    mssim = s / cnt
    if full:
        return mssim, (S if torch.is_tensor(im1) else S.cpu().numpy())
    return mssim


def _tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def ssim_sums_table(fixed, moving, flow, labels=None, num_classes=0, win_size=7, K1=0.01, K2=0.03, registered=None):
    """cf_cine_ssim_table: fixed [H, W, D], moving [T, H, W, D], flow [T, H, W, D, 2] (component 0 along H), labels [H, W, D] or None ->
    (table, registered): table float64 [T, D, 2 + 2 K] = {sum S, count} over the interior of the SSIM map of (frame, slice), then {sum S,
    count} over all pixels with labels == k for each k < K = num_classes (0 without labels); registered the fp32 device tensor [T, D, H, W]
    that was scored: every frame warped onto ED by ONE cf_warp_bilinear_2d call (B = T D), or the `registered` argument (fp32
    [T, H, W, D]; moving and flow are not read then).  Two library calls and one read; the same bits on every run."""
    win = int(win_size)
    fx = _tensor(fixed).to(_dev(), dtype=torch.float64)
    assert fx.dim() == 3, "fixed has to be [H, W, D]"
    H, W, D = fx.shape
    if registered is None:
        m = _tensor(moving).to(_dev(), dtype=torch.float32)
        f = _tensor(flow).to(_dev(), dtype=torch.float32)
        assert m.dim() == 4 and tuple(m.shape[1:]) == (H, W, D), "Shape mismatch: fixed {} and moving {}".format(tuple(fx.shape), tuple(m.shape))
        T = m.shape[0]
        assert tuple(f.shape) == (T, H, W, D, 2), "Shape mismatch: moving {} and flow {}".format(tuple(m.shape), tuple(f.shape))
        f = f.permute(0, 3, 4, 1, 2).reshape(T * D, 2, H, W).contiguous()
        m = m.permute(0, 3, 1, 2).reshape(T * D, 1, H, W).contiguous()
        reg = ops.warp_bilinear(f, m).reshape(T, D, H, W)
    else:
        reg = _tensor(registered).to(_dev(), dtype=torch.float32)
        assert reg.dim() == 4 and tuple(reg.shape[1:]) == (H, W, D), "Shape mismatch: fixed {} and registered {}".format(tuple(fx.shape), tuple(reg.shape))
        T = reg.shape[0]
        reg = reg.permute(0, 3, 1, 2).contiguous()
    fx = fx.permute(2, 0, 1).contiguous()
    K, g = 0, None
    if labels is not None:
        K = int(num_classes)
        g = _tensor(labels).to(_dev())
        assert tuple(g.shape) == (H, W, D), "Shape mismatch: fixed {} and labels {}".format((H, W, D), tuple(g.shape))
        if g.dtype != torch.uint8:
            g = torch.where((g >= 0) & (g < K), g, torch.full_like(g, 255)).to(torch.uint8)
        g = g.permute(2, 0, 1).contiguous()
    cols = 2 + 2 * K
    NP = win * win
    rng = torch.empty(T * D * 2, dtype=torch.float32, device=fx.device)
    part = torch.empty(T * D * (-(-H // 32)) * (-(-W // 64)) * cols, dtype=torch.float64, device=fx.device)
    table = torch.empty(T * D * cols, dtype=torch.float64, device=fx.device)
    check(lib().cf_cine_ssim_table(fx.data_ptr(), _f32(reg), None if g is None else _u8(g), T, D, H, W, K, win, float(K1), float(K2), NP / (NP - 1.0),
                                   rng.data_ptr(), part.data_ptr(), table.data_ptr(), _stream()), "cf_cine_ssim_table")
    return table.cpu().numpy().reshape(T, D, cols), reg


def cine_ssim_table(fixed, moving, flow, labels=None, names=("RV", "MYO", "LV"), win_size=7, K1=0.01, K2=0.03, registered=None,
                    return_registered=False):
    """compute_SSIM.py:74-104 and compute_SSIM_crop_per_structure.py:70-127 for one patient, from one ssim_sums_table visit.

    fixed [H, W, D]: the ED frame's image (scored in fp64); moving [T, H, W, D]: the other frames; flow [T, H, W, D, 2]: their flows onto
    ED (the stacked `flow` arrays of the .npz files, as flow_regularity_table takes them); labels [H, W, D]: the ED segmentation
    (structures = labels 1..len(names)) or None.  Every (frame, slice) is scored against the ED slice with data_range = max - min of the
    registered slice.  registered= (fp32 [T, H, W, D]) takes the place of the warp: the scripts' `'registered' in data.files` branch.

    Returns one dict per (slice, frame), slices outermost like cine_jacobian_table: `SSIM_whole`, the mean of the SSIM map over the
    interior, and with labels `SSIM_rv`, `SSIM_myo`, `SSIM_lv` -- the map's mean over ALL pixels of the structure, NaN where the slice
    has none -- and `SSIM_mean`, their plain mean.  return_registered=True returns (rows, registered): the fp32 [T, H, W, D] images that
    were scored (a device tensor when the image given was one, numpy otherwise)."""
    K = len(names) + 1 if labels is not None else 0
    tab, reg = ssim_sums_table(fixed, moving, flow, labels, K, win_size, K1, K2, registered)
    T, D = tab.shape[:2]
    rows = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(D):
            for t in range(T):
                v = tab[t, d]
                res = {"SSIM_whole": float(v[0] / v[1])}
                if K:
                    per = [float(v[2 + 2 * i] / v[3 + 2 * i]) if v[3 + 2 * i] else float("nan") for i in range(1, K)]
                    for k, s in zip(names, per):
                        res["SSIM_" + k.lower()] = s
                    res["SSIM_mean"] = sum(per) / len(per)
                rows.append(res)
    if return_registered:
        out = reg.permute(0, 2, 3, 1).contiguous()
        return rows, (out if torch.is_tensor(moving if registered is None else registered) else out.cpu().numpy())
    return rows


# ------------------------------------------------------------------------------------------------ compute_contour_metrics.py / get_strain.py
CONTOUR_MODES = ("from_ed", "from_ed_accumulation", "to_ed_accumulation", "to_ed")          # cf_contour_track_table's mode numbers


def contour_counts(counts, D, Pmax, strain=False):
    """counts [D, 3] (endo, epi, RV points per slice) -> contiguous int32 numpy array, checked on the host before any device work"""
    c = np.ascontiguousarray(counts.cpu().numpy() if torch.is_tensor(counts) else counts)
    if c.shape != (D, 3) or c.dtype.kind not in "iu":
        raise ValueError("counts has to be an integer array [D, 3] = %s, got %s %s" % ((D, 3), c.dtype, c.shape))
    if (c < 0).any() or (c.sum(1) > Pmax).any():
        raise ValueError("counts %s: negative, or more points than the padded row of %d" % (c.tolist(), Pmax))
    if strain and (c[:, 0] != c[:, 1]).any():
        d = int(np.argmax(c[:, 0] != c[:, 1]))
        raise ValueError("slice %d: %d endo and %d epi points: strain needs equal counts" % (d, c[d, 0], c[d, 1]))
    return c.astype(np.int32)


def contour_track_table(flow, pts, counts, mode, out=None, counts_dev=None):
    """cf_contour_track_table: flow [D, T, 2, A, B] (ED first, as strain.prepare_flow returns it; frame 0 is never read), pts
    [D, T, Pmax, 2] (0-based ground-truth points in the same frame order: endo, epi, RV, padded), counts [D, 3] on the host, mode a name
    of CONTOUR_MODES or its number -> (pos, table), device tensors: pos fp32 [D, T - 1, Pmax, 2], the tracked positions (from_ed*) or
    predicted deltas (to_ed*) with the bits of chained ops.sample_points calls, and table fp64 [D, T - 1, 3], the mean point error of
    ENDO, EPI, RV per frame in the order strain.contour_tracking_error returns (NaN without points).  One library call whatever T;
    `out` (fp64 device tensor of D (T - 1) 3 elements) receives the table."""
    mode = CONTOUR_MODES.index(mode) if isinstance(mode, str) else int(mode)
    f = _tensor(flow)
    p = _tensor(pts)
    if f.dim() != 5 or f.shape[2] != 2 or p.dim() != 4 or p.shape[3] != 2 or tuple(p.shape[:2]) != tuple(f.shape[:2]):
        raise ValueError("flow has to be [D, T, 2, A, B] and pts [D, T, Pmax, 2], got %s and %s" % (tuple(f.shape), tuple(p.shape)))
    D, T, _, A, B = f.shape
    Pmax = p.shape[2]
    c = contour_counts(counts, D, Pmax)
    f = f.to(_dev(), dtype=torch.float32).contiguous()
    p = p.to(_dev(), dtype=torch.float32).contiguous()
    cd = torch.from_numpy(c).to(f.device) if counts_dev is None else counts_dev
    pos = torch.empty((D, T - 1, Pmax, 2), dtype=torch.float32, device=f.device)
    table = torch.empty(D * (T - 1) * 3, dtype=torch.float64, device=f.device) if out is None else out
    assert table.dtype == torch.float64 and table.numel() == D * (T - 1) * 3 and table.is_contiguous()
    check(lib().cf_contour_track_table(_f32(f), _f32(p), c.ctypes.data, cd.data_ptr(), D, T, A, B, Pmax, mode, _f32(pos), table.data_ptr(), _stream()),
          "cf_contour_track_table")
    return pos, table.view(D, T - 1, 3)


def contour_strain_table(pos, ed_pts, counts, zoom, out=None, counts_dev=None):
    """cf_contour_strain_table: pos fp32 [D, T - 1, Pmax, 2] (contour_track_table's from_ed positions), ed_pts [D, Pmax, 2] (the ED points;
    a view pts[:, 0] of the [D, T, Pmax, 2] array is read in place), counts [D, 3] on the host with equal endo and epi counts, zoom =
    (mm, mm) for the two coordinates -> fp64 device tensor [D, T, 2]: radial and circumferential strain per frame, ED first (row 0 is
    the ED frame against itself).  `out` (fp64, D T 2 elements) receives it."""
    ps = _tensor(pos)
    e = _tensor(ed_pts)
    if ps.dim() != 4 or ps.shape[3] != 2 or e.dim() != 3 or (e.shape[0], e.shape[1], e.shape[2]) != (ps.shape[0], ps.shape[2], 2):
        raise ValueError("pos has to be [D, T - 1, Pmax, 2] and ed_pts [D, Pmax, 2], got %s and %s" % (tuple(ps.shape), tuple(e.shape)))
    D, T, Pmax = ps.shape[0], ps.shape[1] + 1, ps.shape[2]
    c = contour_counts(counts, D, Pmax, strain=True)
    ps = ps.to(_dev(), dtype=torch.float32).contiguous()
    e = e.to(_dev(), dtype=torch.float32)
    if e.stride(2) != 1 or e.stride(1) != 2 or (D > 1 and (e.stride(0) < 2 * Pmax or e.stride(0) % 2)):
        e = e.contiguous()
    stride = e.stride(0) if D > 1 else 2 * Pmax
    cd = torch.from_numpy(c).to(ps.device) if counts_dev is None else counts_dev
    table = torch.empty(D * T * 2, dtype=torch.float64, device=ps.device) if out is None else out
    assert table.dtype == torch.float64 and table.numel() == D * T * 2 and table.is_contiguous()
    check(lib().cf_contour_strain_table(_f32(ps), e.data_ptr(), stride, c.ctypes.data, cd.data_ptr(), D, T, Pmax, float(zoom[0]), float(zoom[1]),
                                        table.data_ptr(), _stream()), "cf_contour_strain_table")
    return table.view(D, T, 2)
