"""Resampled label maps equal the oracle's at every voxel, indicators of exactly 1/2 included (csrc/prev_stage.hip: cf_resize_labels
behind preprocessing._resize_labels, and cf_prev_stage_onehot).

Expected labels: oracle.preprocess.resample_data_or_seg(is_seg=True, order=1, order_z=0) / resize_segmentation(order=1) -- float64
indicators through scipy.ndimage.zoom -- once per case on the CPU (tests/_label_resize_cases.py).  Every assertion is array equality:
no tolerance, no excluded voxels.  The rows are chosen for their ties: on a non-dyadic shape ratio (56 -> 50, 48 -> 43, ...) a straight
label edge has an exact indicator of 1/2 at regular output columns, the float64 chain of the reference falls on one definite side
there, and a decision made on other arithmetic falls on either.  tests/test_label_resize_refs_cpu.py recomputes each case's tie count
and shows that the fp32 decision this project made before differs from the oracle on every tie row.

Routes, each on every case it applies to: preprocessing.resample_data_or_seg (numpy int16 and device float32, with and without a
separate axis), preprocessing.resize_segmentation, preprocessing._resize_labels, ops.prev_stage_onehot (uint8 labels, all axes linear).
Each test prints one line: voxels, exact ties, differing voxels.

Differing voxels measured on an MI355X.  With cf_resize_labels and the float64 sums in cf_prev_stage_onehot: 0 in every case, on every
route.  Before them (one cf_resize3d + cf_assign_where_ge per label behind _resize_labels; fp32 weights and sums inside
cf_prev_stage_onehot) 71 of the 95 tests failed; resample_data_or_seg, resize_segmentation and _resize_labels gave the same count:

    row                      voxels   linear: ties  labels  one-hot   separate: ties  labels
    r56x48_to_50x43            6450            135      36       36              135      36
    r56x48_to_50x42            6300            219      31       30              219      31
    separate_axis_grows       13608            526      10       49              682      10
    separate_last_axis        10750            145      11       14              164      15
    separate_middle_axis       4300             35       7       11               67      17
    labels_from_minus_one      6450            135      28        -              135      28
    all_axes_grow              4500            214       2       19                -       -
    all_axes_shrink             720             41       7        7                -       -
    one_slice                  2150             32      12       12               32      12
    one_line                     42              3       0        0                3       0
    two_d                      2150             17       9        -                -       -
    second_grid_trip        1083600           1852     190      336                -       -
    halving_control            2016            696       0        0              696       0
    doubling_control          32256              0       0        0                0       0"""
import numpy as np
import pytest
import torch

import _label_resize_cases as C

pytestmark = pytest.mark.gpu


def report(route, row, kind, differ):
    """one line per test; differ: boolean mask of the output voxels that are not the oracle's -> their number"""
    print("%s %s / %s: %d voxels, %d exact ties, %d differ" % (route, row, kind, differ.size, C.exact_ties(row, kind), int(differ.sum())))
    return int(differ.sum())


def resample_args(row, kind):
    sep = C.ROWS[row][3]
    return ([sep], True) if kind == "separate" else (None, False)


THREE_D = [c for c in C.CASES if len(C.ROWS[c[0]][0]) == 3]


@pytest.mark.parametrize("row,kind", THREE_D)
def test_resample_data_or_seg_numpy_int16(dev, row, kind):
    from cineflow import preprocessing as P
    seg, expected = C.case(row, kind)
    axis, sep = resample_args(row, kind)
    got = P.resample_data_or_seg(np.stack([seg, seg[::-1]]), C.ROWS[row][1], True, axis, 1, sep, 0)
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == (2,) + expected.shape
    assert report("resample_data_or_seg[int16]", row, kind, got[0] != expected) == 0
    if C.ROWS[row][0][0] == C.ROWS[row][1][0]:                  # second channel: the map flipped along an axis that keeps its samples
        assert np.array_equal(got[1], expected[::-1])


@pytest.mark.parametrize("row,kind", THREE_D)
def test_resample_data_or_seg_tensor_float32(dev, row, kind):
    from cineflow import preprocessing as P
    seg, expected = C.case(row, kind)
    axis, sep = resample_args(row, kind)
    got = P.resample_data_or_seg(torch.tensor(seg[None].astype(np.float32)).to(dev), C.ROWS[row][1], True, axis, 1, sep, 0)
    assert torch.is_tensor(got) and got.dtype == torch.float32 and got.device.type == "cuda"
    assert report("resample_data_or_seg[f32 tensor]", row, kind, got[0].cpu().numpy() != expected) == 0


@pytest.mark.parametrize("row,kind", [c for c in C.CASES if c[1] == "linear"])
def test_resize_segmentation(dev, row, kind):
    """2-D and 3-D maps; numpy int16 in and out, device float32 in and out"""
    from cineflow import preprocessing as P
    seg, expected = C.case(row, kind)
    got = P.resize_segmentation(seg.copy(), C.ROWS[row][1], order=1)
    assert isinstance(got, np.ndarray) and got.dtype == np.int16
    assert report("resize_segmentation[int16]", row, kind, got != expected) == 0
    t = P.resize_segmentation(torch.tensor(seg.astype(np.float32)).to(dev), C.ROWS[row][1], order=1)
    assert torch.is_tensor(t) and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), expected)


@pytest.mark.parametrize("row,kind", THREE_D)
def test_resize_labels(dev, row, kind):
    from cineflow import preprocessing as P
    seg, expected = C.case(row, kind)
    got = P._resize_labels(torch.tensor(seg[None].astype(np.float32)).to(dev), C.ROWS[row][1], C.linear_flags(row, kind))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + expected.shape
    assert report("_resize_labels", row, kind, got[0].cpu().numpy() != expected) == 0


@pytest.mark.parametrize("row,kind", [c for c in C.LINEAR_3D if C.ROWS[c[0]][4] == 0])
def test_prev_stage_onehot(dev, row, kind):
    """uint8 labels, planes of classes 1..3 written behind a guard value; label 0 is the voxels no plane claims"""
    from cineflow import ops
    seg, expected = C.case(row, kind)
    classes = [1, 2, 3]
    out = torch.full((3,) + expected.shape, 7.0, dtype=torch.float32, device=dev)
    ops.prev_stage_onehot(torch.tensor(seg.astype(np.uint8)).to(dev), classes, out)
    planes = np.stack([(expected == c) for c in classes]).astype(np.float32)
    got = out.cpu().numpy()
    assert report("prev_stage_onehot", row, kind, (got != planes).any(0)) == 0
    assert np.array_equal(got, planes)
