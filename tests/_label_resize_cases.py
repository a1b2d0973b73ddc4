"""The label maps of tests/test_gpu_label_resize.py and tests/test_label_resize_refs_cpu.py: seeded Gaussian-smoothed noise quantised to four
equal-volume labels, resampled the way resample_data_or_seg(is_seg=True, order=1) does it.  Expected labels come from
oracle.preprocess alone (float64, scipy), once per case, shared and read-only.

A case is (row, route): route "linear" resizes all axes linearly (do_separate_z=False, resize_segmentation), route "separate" resizes
every slice along the row's separate axis in-plane and takes the nearest slice along it (do_separate_z=True, order_z=0).

COUNTS states for every case what the CPU file recomputes and asserts: the number of output voxels at which some label's exact
indicator is exactly 1/2 (_kernel_refs.label_resize_exact), and the number at which a numpy restatement of cf_resize3d's fp32 chain
thresholded at 0.5f -- the decision this project made before cf_resize_labels -- differs from the oracle.  A row marked `tie` is there
because the second number is positive: an fp32 decision fails it."""
import functools

import numpy as np

# name: (source shape, output shape, seed, separate axis or None, label shift, tie row)
ROWS = {
    "r56x48_to_50x43": ((3, 56, 48), (3, 50, 43), 1, 0, 0, True),
    "r56x48_to_50x42": ((3, 56, 48), (3, 50, 42), 1, 0, 0, True),
    "separate_axis_grows": ((3, 56, 48), (4, 63, 54), 2, 0, 0, True),
    "separate_last_axis": ((48, 56, 3), (43, 50, 5), 1, 2, 0, True),
    "separate_middle_axis": ((56, 3, 48), (50, 2, 43), 1, 1, 0, True),
    "labels_from_minus_one": ((3, 56, 48), (3, 50, 43), 1, 0, -1, True),
    "all_axes_grow": ((6, 14, 10), (9, 20, 25), 4, None, 0, True),
    "all_axes_shrink": ((10, 12, 14), (8, 9, 10), 2, None, 0, True),
    "one_slice": ((1, 56, 48), (1, 50, 43), 1, 0, 0, True),
    "one_line": ((1, 1, 48), (1, 1, 42), 1, 0, 0, False),
    "two_d": ((56, 48), (50, 43), 3, None, 0, True),
    "second_grid_trip": ((3, 56, 48), (9, 400, 301), 1, None, 0, True),       # 1 083 600 voxels > 2^20 threads of the largest grid
    "halving_control": ((3, 56, 48), (3, 28, 24), 1, 0, 0, False),            # dyadic weights: ties that fp32 decides alike
    "doubling_control": ((3, 56, 48), (3, 112, 96), 1, 0, 0, False),          # no indicator of 1/2 at all
}
# (row, route): (voxels with an exact tie, voxels where the fp32 chain's labels differ from the oracle's) -- recomputed by the CPU file
COUNTS = {
    ("r56x48_to_50x43", "linear"): (135, 36),
    ("r56x48_to_50x43", "separate"): (135, 36),
    ("r56x48_to_50x42", "linear"): (219, 31),
    ("r56x48_to_50x42", "separate"): (219, 31),
    ("separate_axis_grows", "linear"): (526, 10),
    ("separate_axis_grows", "separate"): (682, 10),
    ("separate_last_axis", "linear"): (145, 11),
    ("separate_last_axis", "separate"): (164, 15),
    ("separate_middle_axis", "linear"): (35, 8),
    ("separate_middle_axis", "separate"): (67, 17),
    ("labels_from_minus_one", "linear"): (135, 28),
    ("labels_from_minus_one", "separate"): (135, 28),
    ("all_axes_grow", "linear"): (214, 2),
    ("all_axes_shrink", "linear"): (41, 7),
    ("one_slice", "linear"): (32, 12),
    ("one_slice", "separate"): (32, 12),
    ("one_line", "linear"): (3, 0),
    ("one_line", "separate"): (3, 0),
    ("two_d", "linear"): (17, 9),
    ("second_grid_trip", "linear"): (1852, 187),
    ("halving_control", "linear"): (696, 0),
    ("halving_control", "separate"): (696, 0),
    ("doubling_control", "linear"): (0, 0),
    ("doubling_control", "separate"): (0, 0),
}
CASES = sorted(COUNTS)
LINEAR_3D = [c for c in CASES if c[1] == "linear" and len(ROWS[c[0]][0]) == 3]


def smoothed_labels(shape, seed, nlabels=4, sigma=1.5):
    from scipy.ndimage import gaussian_filter
    g = gaussian_filter(np.random.RandomState(seed).randn(*shape), sigma)
    return np.digitize(g, np.quantile(g, np.linspace(0, 1, nlabels + 1)[1:-1])).astype(np.int16)


def linear_flags(row, route):
    src, _dst, _seed, sep, _shift, _tie = ROWS[row]
    return [int(route == "linear" or a != sep) for a in range(len(src))]


@functools.lru_cache(maxsize=None)
def case(row, route):
    """(seg int16, expected labels int16) -- the oracle's resample_data_or_seg / resize_segmentation, computed once"""
    from oracle import preprocess as OP
    src, dst, seed, sep, shift, _tie = ROWS[row]
    seg = smoothed_labels(src, seed) + np.int16(shift)
    assert len(np.unique(seg)) == 4
    if len(src) == 2:
        expected = OP.resize_segmentation(seg, dst, order=1)
    elif route == "linear":
        expected = OP.resample_data_or_seg(seg[None], dst, True, None, 1, False, 0)[0]
    else:
        expected = OP.resample_data_or_seg(seg[None], dst, True, [sep], 1, True, 0)[0]
    assert expected.dtype == np.int16 and expected.shape == tuple(dst)
    for a in (seg, expected):
        a.setflags(write=False)
    return seg, expected


@functools.lru_cache(maxsize=None)
def exact_ties(row, route):
    """number of output voxels where some label's exact indicator is 1/2"""
    import _kernel_refs as R
    seg, _e = case(row, route)
    return int(R.label_resize_exact(seg, ROWS[row][1], linear_flags(row, route))[2].sum())


def fp32_chain_labels(row, route):
    """the decision before cf_resize_labels: per label, ascending, cf_resize3d's fp32 chain of the indicator >= 0.5f"""
    import _kernel_refs as R
    seg, _e = case(row, route)
    dst, lin = tuple(ROWS[row][1]), linear_flags(row, route)
    lead = (1,) * (3 - seg.ndim)
    out = np.zeros(lead + dst, seg.dtype)
    for c in np.unique(seg):
        out[R.resize3d_f32_chain((seg == c).reshape(lead + seg.shape), lead + dst, [1] * len(lead) + lin) >= np.float32(0.5)] = c
    return out.reshape(dst)
