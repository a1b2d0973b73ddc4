"""CPU pins of the label-resize references (tests/_kernel_refs.py linear_chain_f64, labels_from_chain, label_resize_exact) and of the
case table tests/_label_resize_cases.py that tests/test_gpu_label_resize.py runs on the device.  No GPU.

  * linear_chain_f64 IS scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True): every value equal, bit for bit;
  * labels thresholded from it are oracle.preprocess.resize_segmentation's / resample_data_or_seg's, for every case of the table;
  * label_resize_exact's integer sign of indicator - 1/2 agrees with the oracle's `>= 0.5` wherever the indicator is not exactly 1/2;
  * the table's stated counts are what these functions compute, and a tie row is one an fp32 decision gets wrong."""
import numpy as np
import pytest

import _kernel_refs as R
import _label_resize_cases as C


@pytest.mark.parametrize("shape,new", [((56, 48), (50, 43)), ((7, 9), (12, 5)), ((9, 1), (4, 1)), ((3, 56, 48), (3, 50, 43)),
                                       ((1, 56, 48), (1, 50, 43)), ((1, 1, 48), (1, 1, 42)), ((1, 7, 8), (3, 7, 20)),
                                       ((6, 14, 10), (9, 20, 25)), ((10, 12, 14), (8, 9, 10)), ((5, 9, 7), (8, 20, 13))])
def test_chain_is_scipy_zoom_bit_for_bit(shape, new):
    """2-D and 3-D indicators; a one-sample axis (kept and growing), an unchanged axis, growing and shrinking axes"""
    from oracle import preprocess as OP
    seg = C.smoothed_labels(shape, 5)
    n = 0
    for c in np.unique(seg):
        ref = OP.resize((seg == c).astype(float), new, 1, mode="edge", clip=True, anti_aliasing=False)
        got = R.linear_chain_f64(seg == c, new, [1] * len(shape))
        assert got.dtype == np.float64 and np.array_equal(got, ref), "%d of %d values differ" % (int((got != ref).sum()), ref.size)
        n += int(((ref > 0) & (ref < 1)).sum())
    assert n > 0, "no interpolated value: the comparison shows nothing"


@pytest.mark.parametrize("row,route", C.CASES)
def test_chain_labels_are_the_oracles(row, route):
    seg, expected = C.case(row, route)
    got = R.labels_from_chain(seg, C.ROWS[row][1], C.linear_flags(row, route))
    assert got.dtype == expected.dtype and np.array_equal(got, expected), "%d voxels differ" % int((got != expected).sum())


def test_the_separate_routes_are_covered():
    """each of the three axes is the separate one in some case, and in one of them the separate axis changes its size"""
    sep = {C.ROWS[r][3] for r, route in C.CASES if route == "separate"}
    assert sep == {0, 1, 2}
    assert any(C.ROWS[r][0][C.ROWS[r][3]] != C.ROWS[r][1][C.ROWS[r][3]] for r, route in C.CASES if route == "separate")
    assert any(int(np.prod(C.ROWS[r][1])) > 2 ** 20 and C.COUNTS[r, route][0] > 0 for r, route in C.CASES)


@pytest.mark.parametrize("row,route", [c for c in C.CASES if c[0] != "second_grid_trip"])
def test_exact_sign_agrees_with_the_oracle_outside_ties(row, route):
    from oracle import preprocess as OP
    seg, _expected = C.case(row, route)
    dst, lin = C.ROWS[row][1], C.linear_flags(row, route)
    labels, sign, tie, gap = R.label_resize_exact(seg, dst, lin)
    assert gap > 1e-9, "an indicator is closer to 1/2 than the fp64 chain can resolve"       # (the chain's error is a few 1e-16)
    for j, c in enumerate(labels):
        if route == "linear":
            ind = OP.resize((seg == c).astype(float), dst, 1, mode="edge", clip=True, anti_aliasing=False)
        else:
            ind = R.linear_chain_f64(seg == c, dst, lin)              # (pinned to the oracle by the two tests above)
        away = sign[j] != 0
        assert np.array_equal((ind >= 0.5)[away], (sign[j] > 0)[away])
        assert float(np.abs(ind[~away] - 0.5).max(initial=0.0)) < 1e-14
    assert tie.shape == tuple(dst) and np.array_equal(tie, (sign == 0).any(0))


@pytest.mark.parametrize("row,route", C.CASES)
def test_stated_counts_and_tie_rows_can_fail(row, route):
    seg, expected = C.case(row, route)
    tie = R.label_resize_exact(seg, C.ROWS[row][1], C.linear_flags(row, route))[2]
    differs = C.fp32_chain_labels(row, route) != expected
    print("%s / %s: %d voxels, %d exact ties, fp32 chain differs at %d" % (row, route, expected.size, int(tie.sum()), int(differs.sum())))
    assert (int(tie.sum()), int(differs.sum())) == C.COUNTS[row, route]
    assert not (differs & ~tie).any(), "the fp32 chain differs from the oracle away from a tie"
    if C.ROWS[row][5]:
        assert tie.any() and differs.any(), "sold as a tie row, but an fp32 decision passes it"


def test_cf_resize_labels_is_declared_bound_and_exported():
    import ctypes
    import os
    import re
    import torch
    from cineflow import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cineflow.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+cf_resize_labels\s*\(", header)
    P_, I_ = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["cf_resize_labels"] == [P_, P_] + [I_] * 10 + [P_]
    h = _lib.lib()
    # argument errors are caught on the host, before any launch
    assert h.cf_resize_labels(None, 16, 1, 4, 4, 4, 8, 8, 8, 1, 1, 1, None) == -1 and b"null or aliased" in h.cf_last_error()
    assert h.cf_resize_labels(16, 16, 1, 4, 4, 4, 8, 8, 8, 1, 1, 1, None) == -1 and b"null or aliased" in h.cf_last_error()
    assert h.cf_resize_labels(16, 32, 1, 4, 4, 4, 8, 0, 8, 1, 1, 1, None) == -1 and b"bad shape" in h.cf_last_error()
    with pytest.raises(TypeError):
        ops.resize_labels(torch.zeros(1, 4, 4, 4), (8, 8, 8))                        # CPU tensors: no CPU path
