"""csrc/score.hip against the oracle: cf_label_surface_count / cf_label_surface_table (all frames and classes of a patient in one
visit) per (frame, class) against oracle.metrics.medpy_binary.surface_distances and ConfusionMatrix on the masks `label == c`, and
cf_flow_regularity_table per (slice, frame) against oracle.metrics.jacobian_frame_stats / gradient_means.

Bars.  Surface table: those of tests/test_gpu_metrics_kernels.py -- counts and border counts identical, every sorted distance within
1e-12, the maxima exactly the largest distance, the device sums within n * 2^-53 * sum (an fp64 sum in any order); the scores of
cine_label_scores within 1e-12 of the oracle's functions, NaN where they are NaN.  Flow table: those of
tests/test_metrics.py::test_metrics_device -- means 1e-4, gradient means 1e-6, percentages 0.5, counts within the number of oracle
determinants within 2e-5 of zero in that slice (<= 2 for every input here, asserted).

Measured on the MI355X (pytest -s prints one line per row: worst figure, bar, ratio):
  surface table (10 rows, up to 4,422 border points): counts identical, sorted distances identical (worst 0), device sums <= 0.29 of their bars
  flow table (5 rows): counts identical, gradient means identical, means within 4.5e-16, the table bit-identical between two calls
"""
import numpy as np
import pytest
import torch

from cineflow._lib import CineflowError
from _kernel_refs import ratio_line, surface_border
from _score_refs import check_jacobian_row, jacobian_rows, smooth_flow, structure_labels

pytestmark = pytest.mark.gpu

SP = (7.5, 0.9, 1.3)


# ------------------------------------------------------------------------------------------------ cf_label_surface_table
def _even_points(rng, counts, shape=(20, 40, 50)):
    """a label volume with counts[c - 1] voxels of class c, all on even coordinates: each voxel is its own border voxel"""
    grid = np.stack(np.meshgrid(*[np.arange(0, s, 2) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    sel = grid[rng.choice(len(grid), sum(counts), replace=False)]
    lab = np.zeros(shape, np.uint8)
    lo = 0
    for c, k in enumerate(counts, 1):
        p = sel[lo:lo + k]
        lab[p[:, 0], p[:, 1], p[:, 2]] = c
        lo += k
    return lab


def _blobs(rng, shape, levels=(0.25, 0.6, 0.85)):
    """smooth noise cut into labels 0..3: connected regions of different sizes, touching each other and the array's faces"""
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(rng.normal(size=shape), 1.6)
    f = (f - f.min()) / (f.max() - f.min())
    return np.digitize(f, np.quantile(f, levels)).astype(np.uint8)


def surface_cases():
    c = {}
    one_t, one_r = np.zeros((1, 3, 5, 6), np.uint8), np.zeros((1, 3, 5, 6), np.uint8)
    one_t[0, 0, 0, 0], one_t[0, 1, 2, 3], one_t[0, 2, 4, 5] = 1, 2, 3
    one_r[0, 2, 4, 0], one_r[0, 1, 2, 4], one_r[0, 0, 0, 5] = 1, 2, 3
    c["N = 1, one voxel per class"] = (one_t, one_r)
    rng = np.random.default_rng(255)
    c["segments of 255 / 256 / 257 border points"] = (_even_points(rng, (255, 256, 257))[None], _even_points(rng, (257, 255, 256))[None])
    rng = np.random.default_rng(3)
    c["N = 3, unequal segments"] = (np.stack([_blobs(rng, (4, 18, 16), q) for q in ((0.25, 0.6, 0.85), (0.5, 0.7, 0.95), (0.1, 0.3, 0.5))]),
                                    np.stack([_blobs(rng, (4, 18, 16), q) for q in ((0.3, 0.5, 0.9), (0.2, 0.8, 0.9), (0.4, 0.5, 0.6))]))
    t, r = _blobs(rng, (3, 9, 11))[None], _blobs(rng, (3, 9, 11))[None]
    t[t == 1] = 0                                                                    # class 1: in the reference only
    r[r == 2] = 0                                                                    # class 2: in the test only
    c["a class absent in test only, in reference only, in both"] = (np.concatenate([t, np.where(t == 3, 0, t)]), np.concatenate([r, np.where(r == 3, 0, r)]))
    full = np.ones((1, 3, 6, 7), np.uint8)
    part = np.zeros((1, 3, 6, 7), np.uint8)
    part[0, 1:, 2:5, 1:4] = 1
    c["a class that fills the volume"] = (np.concatenate([full, part, full]), np.concatenate([part, full, full]))
    blob_t, blob_r = np.zeros((9, 11), np.uint8), np.zeros((9, 11), np.uint8)
    blob_t[1:8, 2:10], blob_t[0, 4:6], blob_t[3:5, 4:7] = 1, 1, 2
    blob_r[2:9, 1:8], blob_r[4:7, 3:6] = 1, 2
    c["a blob as (1, H, W) with ndim = 3: every voxel is border"] = (blob_t[None, None], blob_r[None, None])
    c["the same blob as (H, W) with ndim = 2"] = (blob_t[None], blob_r[None])
    touch_t, touch_r = np.zeros((1, 2, 8, 10), np.uint8), np.zeros((1, 2, 8, 10), np.uint8)
    touch_t[0, :, 1:7, 1:5], touch_t[0, :, 1:7, 5:9] = 1, 2                          # the two classes share a face: column 4 | column 5
    touch_r[0, :, 2:8, 0:4], touch_r[0, :, 2:8, 4:9], touch_r[0, 1, 4, 4:6] = 1, 2, 3
    c["two touching classes"] = (touch_t, touch_r)
    edge_t, edge_r = np.zeros((2, 3, 6, 6), np.uint8), np.zeros((2, 3, 6, 6), np.uint8)
    edge_t[0, 1:, 1:5, 1:5], edge_t[1, :2, 1:5, 1:5] = 1, 1                          # frame 0 ends on its last plane, frame 1 starts on its first
    edge_r[0, 2, 2:6, 0:4], edge_r[1, 0, 2:6, 0:4] = 1, 1
    c["an object on the last plane of frame n, one on the first plane of frame n + 1"] = (edge_t, edge_r)
    rows_t, rows_r = np.zeros((2, 6, 7), np.uint8), np.zeros((2, 6, 7), np.uint8)
    rows_t[0, 4:, 1:6], rows_t[1, :2, 1:6] = 2, 2                                     # the same for 2-D frames: last rows, first rows
    rows_r[0, 5, 0:5], rows_r[1, 0, 2:7] = 2, 2
    c["2-D frames: last rows of frame n, first rows of frame n + 1"] = (rows_t, rows_r)
    return c


@pytest.mark.parametrize("tag", list(surface_cases()))
def test_label_surface_table(dev, tag):
    from cineflow import metrics as M
    from oracle import metrics as OM
    test, ref = surface_cases()[tag]
    K = 4
    nd = test.ndim - 1
    sp = SP[3 - nd:]
    tab, dist, offs = M.label_surface_table(torch.from_numpy(test).to(dev), ref, K, sp)
    N = len(test)
    assert tab.shape == (N, K, 9) and offs.shape == (N, K, 2, 2) and not tab[:, 0].any()
    scores = M.cine_label_scores(test, ref, K, sp)
    loose = M.cine_label_scores(test, ref, K, sp, reproducible=False)
    worst_d = worst_s = 0.0
    lo = 0
    segments = set()
    for n in range(N):
        for c in range(1, K):
            a, b = test[n] == c, ref[n] == c
            tp, fp, tn, fn = OM.ConfusionMatrix(a, b).get_matrix()
            assert tuple(tab[n, c, :3]) == (tp, fp, fn), (tag, n, c)
            na, nb = (len(surface_border(m)) if m.any() else 0 for m in (a, b))
            assert tuple(tab[n, c, 3:5]) == (na, nb), (tag, n, c)
            for side, cnt in ((0, na), (1, nb)):                                     # the segments tile the buffer in order
                assert tuple(offs[n, c, side]) == (lo, lo + cnt), (tag, n, c, side)
                segments.add((lo, cnt))
                lo += cnt
            if na and nb:
                for side, (x, y) in enumerate(((a, b), (b, a))):
                    want = np.sort(OM.medpy_binary.surface_distances(x, y, sp))
                    got = dist[offs[n, c, side, 0]:offs[n, c, side, 1]]
                    assert got.shape == want.shape
                    worst_d = max(worst_d, float(np.abs(np.sort(got) - want).max()))
                    assert tab[n, c, 5 + side] == got.max(), (tag, n, c, side)           # the maximum is exact
                    err, bar = abs(tab[n, c, 7 + side] - got.sum()), len(got) * 2.0 ** -53 * got.sum()
                    worst_s = max(worst_s, err / bar if bar else err)
                    assert err <= bar, (tag, n, c, side, err, bar)
            else:
                assert not tab[n, c, 5:].any()
            want = {"dice": OM.dice(a, b), "hd": OM.hausdorff_distance(a, b, voxel_spacing=sp),
                    "asd_test_to_ref": OM.avg_surface_distance(a, b, voxel_spacing=sp), "asd_ref_to_test": OM.avg_surface_distance(b, a, voxel_spacing=sp),
                    "assd": OM.avg_surface_distance_symmetric(a, b, voxel_spacing=sp), "hd95": OM.hausdorff_distance_95(a, b, voxel_spacing=sp)}
            for k, w in want.items():
                for got in (scores[k][n, c], loose[k][n, c]):
                    assert (np.isnan(got) and np.isnan(w)) or abs(got - w) <= 1e-12, (tag, n, c, k, got, w)
    assert lo == len(dist)
    assert all(np.isnan(v[:, 0]).all() for v in scores.values())
    print()
    ratio_line("surface table: %s (%d points)" % (tag[:34], len(dist)), worst_d, 1e-12)
    ratio_line("surface table: device sums / their bars", worst_s, 1.0)
    assert worst_d <= 1e-12
    if tag == "N = 3, unequal segments":
        starts, sizes = sorted(lo for lo, _ in segments), [cnt for _, cnt in segments]
        assert len(starts) == 18 and min(sizes) > 0 and len(set(sizes)) > 9, (starts, sizes)      # every offset past the first non-zero, all unequal
    if tag.startswith("segments of 255"):
        assert sorted(tab[0, 1:, 3]) == [255, 256, 257] and sorted(tab[0, 1:, 4]) == [255, 256, 257]
    if tag.startswith("a class that fills"):
        assert np.isnan(scores["hd"][:, 1]).all() and not np.isnan(scores["dice"][:, 1]).any() and tab[0, 1, 3] == 3 * 6 * 7 - 4 * 5
    if tag.startswith("a blob as (1, H, W)"):
        assert tab[0, 1, 3] == (test == 1).sum() and tab[0, 2, 3] == (test == 2).sum()
    if tag.startswith("the same blob as (H, W)"):
        assert tab[0, 1, 3] < (test == 1).sum()


def test_label_surface_table_reports_labels_past_K(dev):
    from cineflow import metrics as M
    test, ref = (a.copy() for a in surface_cases()["two touching classes"])
    M.label_surface_table(test, ref, 4)
    for which in (0, 1):
        bad = [test.copy(), ref.copy()]
        bad[which][0, 1, 7, 9] = 4
        with pytest.raises(ValueError, match="1 voxels carry a label >= num_classes=4"):
            M.label_surface_table(bad[0], bad[1], 4)
        with pytest.raises(ValueError, match="label >= num_classes"):
            M.cine_label_scores(bad[0], bad[1], 4)
    assert M.label_surface_table(test, ref, 16)[0].shape == (1, 16, 9)
    with pytest.raises(CineflowError, match="K must be"):
        M.label_surface_table(test, ref, 17)


def test_label_surface_table_empty_stack(dev):
    """no foreground anywhere: no border point, no distance launch, NaN scores"""
    from cineflow import metrics as M
    z = np.zeros((2, 5, 6), np.uint8)
    tab, dist, offs = M.label_surface_table(z, z, 4)
    assert not tab.any() and dist.size == 0 and not offs.any()
    assert all(np.isnan(v).all() for v in M.cine_label_scores(z, z, 4).values())


# ------------------------------------------------------------------------------------------------ cf_flow_regularity_table
FLOW_CASES = {
    "(1, 2, 2, 1): the temporal gradient is 0": dict(shape=(1, 2, 2, 1), seed=1, amp=0.5),
    "(2, 5, 7, 2)": dict(shape=(2, 5, 7, 2), seed=2, amp=0.5),
    "(3, 33, 65, 3): past one tile in both axes": dict(shape=(3, 33, 65, 3), seed=3, amp=0.5),
    "(2, 9, 12, 2): a structure absent in one frame": dict(shape=(2, 9, 12, 2), seed=4, amp=0.5, absent=2),
    "(2, 40, 70, 2): amplitude 2 px, negatives exist": dict(shape=(2, 40, 70, 2), seed=5, amp=2.0),
}


def _flow_case(shape, seed, amp, absent=None):
    T, H, W, D = shape
    rng = np.random.default_rng(seed)
    flow = smooth_flow(rng, T, H, W, D, amp)
    lab = structure_labels(rng, (T, H, W, D))
    if H * W <= 4:
        lab[:, 0, 0], lab[:, 0, 1], lab[:, 1, 0] = 1, 2, 3                           # four pixels: one per structure
    if absent is not None:
        lab[0][lab[0] == absent] = 0
    return flow, lab


@pytest.mark.parametrize("tag", list(FLOW_CASES))
def test_flow_regularity_table(dev, tag):
    from cineflow import metrics as M
    flow, lab = _flow_case(**FLOW_CASES[tag])
    T, H, W, D, _ = flow.shape
    want, near = jacobian_rows(flow, lab)
    assert max(near) <= 2, near                                                      # the inputs keep the count bar tight (host-only check)
    got = M.cine_jacobian_table(flow, lab)
    assert len(got) == len(want) == D * T
    assert list(got[0]) == list(want[0]) and list(got[0])[:2] == ["Temporal gradient", "Spatial gradient"]
    worst = {}
    for i, (g, w) in enumerate(zip(got, want)):
        for k, v in check_jacobian_row(g, w, near[i], "%s slice %d frame %d" % (tag, i // T, i % T)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print()
    for k, bar in (("mean", 1e-4), ("gradient", 1e-6), ("percent", 0.5), ("count", 2)):
        ratio_line("flow table %s: %s" % (tag[:16], k), worst[k], bar)
    tab = M.flow_regularity_table(torch.from_numpy(flow).to(dev), torch.from_numpy(lab).to(dev), 4)
    assert tab.shape == (T, D, 17) and np.array_equal(tab[:, :, 15], np.full((T, D), H * W))
    assert np.array_equal(tab[:, :, 3:13:3].sum(-1), tab[:, :, 15])       # the labels partition the slice
    assert np.array_equal(tab, M.flow_regularity_table(flow, lab, 4))                  # the same bits on every run
    if T == 1:
        assert not tab[:, :, 0].any()
    if "absent" in tag:
        assert np.isnan(got[0]["abs(Mean jacobian - 1)_MYO"]) and np.isnan(got[0]["negative_%_average"]) and got[0]["total_MYO"] == 0.0
        assert not np.isnan(got[1]["abs(Mean jacobian - 1)_MYO"])
    if "negatives" in tag:
        assert min(r["negative"] for r in want) > 0 and sum(r["negative_LV"] for r in want) > 0


def test_flow_regularity_ignores_labels_past_K_and_accepts_wide_dtypes(dev):
    from cineflow import metrics as M
    flow, lab = _flow_case((2, 9, 12, 2), 6, 0.5)
    wide = lab.astype(np.int16)
    wide[0, 0, 0, 0], wide[1, 2, 3, 1] = 300, -1                                       # neither is a structure; both count for the whole slice
    as_u8 = lab.copy()
    as_u8[0, 0, 0, 0], as_u8[1, 2, 3, 1] = 200, 9
    a, b = M.flow_regularity_table(flow, wide, 4), M.flow_regularity_table(flow, as_u8, 4)
    assert np.array_equal(a, b) and np.array_equal(a[:, :, 15], np.full((2, 2), 9 * 12))
    assert a[0, 0, 3:13:3].sum() == 9 * 12 - 1
    with pytest.raises(CineflowError, match="two points per axis"):
        M.flow_regularity_table(flow[:, :1], lab[:, :1], 4)
