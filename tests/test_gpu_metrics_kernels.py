"""Operator-level tables for csrc/metrics.hip: every kernel against numpy / scipy restatements (tests/_kernel_refs.py) or the oracle, at
one element, around a block or a tile, past the second grid-stride trip of its launch, and on the cases a single fixture cannot pin
(an object that fills the array, a one-voxel plate, the z-face rule of a one-slice volume, labels past K, +-0.0).

Bars.  Counts and border sets: identical.  Surface distances: the project's 1e-12 against oracle.metrics.medpy_binary on sorted
values.  fp64 sums (cf_max_sum_nonneg, cf_region_stats): n * 2^-53 * sum|x|, the worst case of an fp64 sum in any order; maxima exact.
spatial_gradient3d 1e-7, gradient_means 1e-6, SSIM 1e-10 (score) / 1e-9 (map): the bars test_metrics.py already holds them to.

Measured on the MI355X (pytest -s prints one line per row: worst figure, bar, ratio):
  confusion (6 rows) and border sets (7 rows, up to 607,048 border voxels): identical
  surface distances (35 rows): worst 1.42e-14 (nA = 255, nB = 1), ratio 0.014
  cf_max_sum_nonneg, cf_region_stats: maxima and counts exact, sums <= 0.001 of their bars
  spatial_gradient3d, gradient_means: 0 (the same fp32 operations); SSIM score 6.4e-15, map 2.7e-14
"""
import numpy as np
import pytest
import torch

from _kernel_refs import confusion, ratio_line, region_stats, surface_border

pytestmark = pytest.mark.gpu

N20 = 17 * 251 * 247                  # 1,053,949 > 2^20
N24 = 65 * 509 * 509                  # 16,840,265 > 2^24: the second trip of the 16-per-thread reductions


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ ConfusionMatrix / label_confusion
@pytest.fixture(scope="module")
def label_pair():
    rng = np.random.default_rng(31)
    return rng.integers(0, 16, N24, dtype=np.uint8), rng.integers(0, 16, N24, dtype=np.uint8)


@pytest.mark.parametrize("n", [1, 4097, N24])
@pytest.mark.parametrize("K", [4, 16])
def test_confusion_table(dev, label_pair, n, K):
    from cineflow import metrics as M
    t, r = (a[N24 - n:] % K for a in label_pair)
    want = confusion(t, r, K)
    td, rd = torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev)
    got = M.label_confusion(td, rd, K)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    cm = M.ConfusionMatrix(td, rd)
    tp, fp, fn = int(want[1:, 1:].sum()), int(want[1:, 0].sum()), int(want[0, 1:].sum())
    assert cm.get_matrix() == (tp, fp, n - tp - fp - fn, fn) and cm.get_size() == n
    assert cm.get_existence() == (tp + fp == 0, tp + fp == n, tp + fn == 0, tp + fn == n)
    print()
    ratio_line("confusion n=%d K=%d: differing counts" % (n, K), float((got != want).sum()), 0)
    if K < 16:                                                           # labels >= K are reported, not counted
        bad = t.copy()
        bad[-1] = K
        with pytest.raises(ValueError, match="label >= num_classes"):
            M.label_confusion(torch.from_numpy(bad).to(dev), rd, K)
        with pytest.raises(ValueError, match="label >= num_classes"):
            M.label_confusion(rd, torch.from_numpy(bad).to(dev), K)


def test_confusion_existence_flags(dev):
    from cineflow import metrics as M
    e, f = np.zeros(4097, np.uint8), np.ones(4097, np.uint8)
    assert M.ConfusionMatrix(e, f).get_existence() == (True, False, False, True) and M.ConfusionMatrix(e, f).get_matrix() == (0, 0, 0, 4097)
    assert M.ConfusionMatrix(f, e).get_existence() == (False, True, True, False) and M.ConfusionMatrix(f, e).get_matrix() == (0, 4097, 0, 0)


# ------------------------------------------------------------------------------------------------ _border + surface_distances
def _border_rows(dev, mask):
    from cineflow import metrics as M
    co, n = M._border(torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev))
    co = co[:3 * n].cpu().numpy().reshape(n, 3)
    return co[np.lexsort(co.T[::-1])]


def border_cases():
    c = {}
    c["object fills the array"] = np.ones((4, 5, 6), bool)
    plate = np.zeros((5, 9, 8), bool)
    plate[2, 1:8, 2:7] = True
    c["one-voxel plate"] = plate
    blob = np.zeros((9, 11), bool)
    blob[1:8, 2:10] = True
    blob[0, 4:6] = True                                                  # touches the array edge
    c["2-D blob"] = blob
    c["the same blob as (1, H, W): every voxel is border"] = blob[None]
    c["2-D full"] = np.ones((5, 7), bool)
    rng = np.random.default_rng(41)
    big = rng.random((17, 251, 247)) < 0.6                               # > 2^20 voxels: the border flags of the second trip
    c["17 x 251 x 247 noise"] = big
    odd = rng.random((3, 7, 9)) < 0.7                                    # 189 voxels: the last wave is ragged (n rounds up to 192)
    c["3 x 7 x 9 noise"] = odd
    return c


def test_surface_border_table(dev):
    print()
    for tag, m in border_cases().items():
        got, want = _border_rows(dev, m), surface_border(m)
        ratio_line("border: %s (%d voxels)" % (tag, len(want)), float(len(got) != len(want) or (got != want).sum()), 0)
        assert got.shape == want.shape and np.array_equal(got, want), tag
    c = border_cases()
    assert len(surface_border(c["object fills the array"])) == 120 - 2 * 3 * 4
    assert len(surface_border(c["one-voxel plate"])) == c["one-voxel plate"].sum()
    assert len(surface_border(c["the same blob as (1, H, W): every voxel is border"])) == c["2-D blob"].sum() > len(surface_border(c["2-D blob"]))


def _points(rng, k, shape=(20, 40, 50)):
    """k voxels on even coordinates: each is its own border voxel"""
    grid = np.stack(np.meshgrid(*[np.arange(0, s, 2) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    m = np.zeros(shape, bool)
    sel = grid[rng.choice(len(grid), k, replace=False)]
    m[sel[:, 0], sel[:, 1], sel[:, 2]] = True
    return m


COUNTS = (1, 255, 256, 257, 4999)


@pytest.mark.parametrize("nA", COUNTS)
def test_surface_distances_tile_boundaries(dev, nA):
    """border sets of exactly nA and nB points around the 256-point tiles of surface_min_dist_kernel, anisotropic spacing"""
    from cineflow import metrics as M
    from oracle import metrics as OM
    sp = (7.5, 0.9, 1.3)
    rng = np.random.default_rng(nA)
    a = _points(rng, nA)
    print()
    for nB in COUNTS:
        b = _points(rng, nB)
        want = np.sort(OM.medpy_binary.surface_distances(a, b, sp))
        got = np.sort(M.surface_distances(a, b, sp).cpu().numpy())
        assert got.shape == want.shape == (nA,)
        worst = float(np.abs(got - want).max())
        ratio_line("surface distances nA=%d nB=%d" % (nA, nB), worst, 1e-12)
        assert worst <= 1e-12


@pytest.mark.parametrize("tag", ["object fills the array", "one-voxel plate", "2-D blob", "the same blob as (1, H, W): every voxel is border", "3 x 7 x 9 noise"])
def test_surface_distances_shapes(dev, tag):
    from cineflow import metrics as M
    from oracle import metrics as OM
    a = border_cases()[tag]
    b = np.zeros_like(a)
    b[tuple(slice(s // 3, s // 3 + max(s // 2, 1)) for s in a.shape)] = True
    sp = (7.5, 0.9, 1.3)[3 - a.ndim:]
    print()
    for x, y in ((a, b), (b, a)):
        want = np.sort(OM.medpy_binary.surface_distances(x, y, sp))
        got = np.sort(M.surface_distances(x, y, sp).cpu().numpy())
        assert got.shape == want.shape
        worst = float(np.abs(got - want).max())
        ratio_line("surface distances: " + tag, worst, 1e-12)
        assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------ _max_sum
@pytest.mark.parametrize("n", [1, 4097, N20])
def test_max_sum_table(dev, n):
    from cineflow import metrics as M
    x = np.abs(np.random.default_rng(n).normal(size=n)) * 30.0
    x[-1] = 200.0                                                        # the maximum sits in the last element
    mx, sm = M._max_sum(torch.from_numpy(x).to(dev))
    bar = n * 2.0 ** -53 * x.sum()
    print()
    ratio_line("max_sum n=%d: sum" % n, abs(sm - x.sum()), bar)
    assert mx == 200.0 and abs(sm - x.sum()) <= bar
    assert M._max_sum(torch.zeros(n, dtype=torch.float64, device=dev)) == (0.0, 0.0)


# ------------------------------------------------------------------------------------------------ cf_region_stats
@pytest.mark.parametrize("n", [1, 4097, N20])
@pytest.mark.parametrize("K", [1, 16])
def test_region_stats_table(dev, n, K):
    from cineflow._lib import check, lib
    rng = np.random.default_rng(n + K)
    x = rng.normal(size=n) * 3.0 + 1.0
    x[::7], x[3::11] = 0.0, -0.0                                         # neither zero is negative
    lab = rng.choice(np.array(list(range(17)) + [200, 255], np.uint8), size=n)                 # 16, 200, 255: ignored at every K
    lab[-1] = K - 1
    want = region_stats(x, lab, K)
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    st = torch.full((3 * K,), float("nan"), dtype=torch.float64, device=dev)
    check(lib().cf_region_stats(xd.data_ptr(), ld.data_ptr(), n, K, st.data_ptr(), _stream()), "cf_region_stats")
    got = st.cpu().numpy().reshape(K, 3)
    assert np.array_equal(got[:, 1], want[:, 1]) and np.array_equal(got[:, 2], want[:, 2]), (got, want)
    bar = n * 2.0 ** -53 * want[:, 3]
    err = np.abs(got[:, 0] - want[:, 0])
    k = int(np.argmax(err - bar))
    print()
    ratio_line("region_stats n=%d K=%d: sum (worst label %d)" % (n, K, k), err[k], bar[k])
    assert (err <= bar).all(), (err, bar)
    assert want[:, 1].sum() == (lab < K).sum()


# ------------------------------------------------------------------------------------------------ gradients and SSIM
@pytest.mark.parametrize("shape", [(1, 2, 1, 5, 6), (1, 2, 2, 5, 6), (2, 1, 4, 1, 6), (2, 1, 4, 2, 6), (1, 1, 4, 5, 1), (1, 1, 4, 5, 2), (1, 1, 1, 1, 1),
                                   (3, 2, 17, 251, 83)])
def test_spatial_gradient3d_thin_axes(dev, shape):
    """an axis of extent 1 has a zero gradient (both replicate-padded neighbours are the voxel itself), extent 2 a one-sided half difference"""
    from cineflow import metrics as M
    from oracle import metrics as OM
    x = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32)
    got, want = M.spatial_gradient3d(x), OM.spatial_gradient3d(x)
    worst = float(np.abs(got - want).max())
    print()
    ratio_line("spatial_gradient3d %s" % (shape,), worst, 1e-7)
    assert got.shape == want.shape and worst <= 1e-7
    for comp, ax in ((0, 4), (1, 3), (2, 2)):
        if shape[ax] == 1:
            assert not got[:, :, comp].any()
        if shape[ax] == 2:
            half = 0.5 * np.diff(x, axis=ax)
            assert np.array_equal(got[:, :, comp], np.concatenate([half, half], ax))


@pytest.mark.parametrize("T,H,W", [(1, 5, 6), (2, 5, 6), (4, 1, 6), (4, 2, 6), (4, 5, 1), (4, 5, 2), (3, 130, 70)])
def test_gradient_means_thin_axes(dev, T, H, W):
    from cineflow import metrics as M
    from oracle import metrics as OM
    flow = np.random.default_rng(T * H * W).normal(size=(T, H, W, 2)).astype(np.float32) * 2.0
    tg, sg = M.gradient_means(flow)
    wt, ws = OM.gradient_means(flow)
    worst = max(float(np.abs(tg - wt).max()), float(np.abs(sg - ws).max()))
    print()
    ratio_line("gradient_means T=%d H=%d W=%d" % (T, H, W), worst, 1e-6)
    assert tg.shape == wt.shape == (T,) and sg.shape == ws.shape == (T,) and worst <= 1e-6


@pytest.mark.parametrize("H,W,win", [(7, 7, 7), (7, 12, 7), (12, 7, 7), (9, 11, 9), (3, 3, 3), (3, 40, 3), (11, 11, 11)])
def test_ssim_window_reaches_image_size(dev, H, W, win):
    from cineflow import metrics as M
    from oracle import metrics as OM
    rng = np.random.default_rng(H * W + win)
    a = rng.normal(size=(H, W)) * 40 + 300
    b = a + rng.normal(size=(H, W)) * 12
    dr = b.max() - b.min()
    want, wmap = OM.structural_similarity(a, b, data_range=dr, win_size=win, full=True)
    got, gmap = M.structural_similarity(a, b, data_range=dr, win_size=win, full=True)
    print()
    ratio_line("ssim %dx%d win %d: score" % (H, W, win), abs(got - want), 1e-10)
    ratio_line("ssim %dx%d win %d: map" % (H, W, win), float(np.abs(gmap - wmap).max()), 1e-9)
    assert abs(got - want) <= 1e-10 and float(np.abs(gmap - wmap).max()) <= 1e-9
    with pytest.raises(ValueError):
        M.structural_similarity(a, b, data_range=dr, win_size=win + 2)
