"""csrc/edt.hip on the device: cineflow.metrics.distance_transform_edt against scipy.ndimage.distance_transform_edt, the "edt" route of
surface_distances against the all-pairs route and against scipy's map gathered at the border, label_surface_edt_table against the per-label
metric functions on the pairs route, normalized_surface_dice against the formula on scipy's distances.  scipy and the pairs route are the
references; nothing here is compared with itself except the two runs that must be byte-identical.

The bound where the spacing is not dyadic
-----------------------------------------
A distance is sqrt(fl(fl(a + b) + c)) with a = fl((sz dz)^2), b = fl((sy dy)^2), c = fl((sx dx)^2), minimised over the zero voxels.  With
dyadic spacings (1; 2.5 and 0.78125 = 25/32; 3 and 1.25) every product and sum is exact in fp64 at these extents, the minimum is the
minimum of exact numbers, and every correct transform returns the same bits: those cases are compared with ==.  With (1.37, 0.7, 0.7) each
candidate's squared distance carries the roundings of the expression -- at most three in sequence on any term (product, square, and the
sums; (1 + u)^3 with u = 2^-53) -- so two candidates whose true squared distances differ by less than those roundings may be ranked
either way by two correct implementations that round in different places (scipy ranks with the parabola intersections of its feature
transform, the kernels with partial sums in y, x order).  Whichever of the two is picked, the value returned is the expression on that
candidate: it differs from the other's by at most the ranking slack plus its own roundings, about 8 u = 2^-50 of the squared distance,
and the square root halves a relative error.  2^-50 on the distance itself is therefore a bound with a factor two to spare; the largest
value seen is in profiles/edt_table.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EXACT = [(1.0, 1.0, 1.0), (2.5, 0.78125, 0.78125), (3.0, 1.25, 1.25)]
ROUNDED = (1.37, 0.7, 0.7)
REL = 2.0 ** -50
SHAPES = [(7, 5), (1, 7, 5), (3, 70, 67), (5, 33, 130), (65, 9, 3), (2, 129, 257)]


def masks(shape, seed):
    """seeded random at 3 % zeros; a single zero in a corner; a zero plane; all zeros but one voxel"""
    rng = np.random.default_rng(seed)
    out = [("random", rng.random(shape) >= 0.03)]
    m = np.ones(shape, bool)
    m[(-1,) * len(shape)] = False
    out.append(("corner", m))
    m = np.ones(shape, bool)
    m[(slice(None),) * (len(shape) - 2) + (shape[-2] // 2,)] = False
    out.append(("plane", m))
    m = np.zeros(shape, bool)
    m[tuple(s // 3 for s in shape)] = True
    out.append(("one voxel", m))
    if out[0][1].all():
        out[0][1].flat[rng.integers(out[0][1].size)] = False
    return out


def rel_err(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(want, 1e-300) * (want > 0))) if want.size else 0.0


def compare(got, want, exact, what):
    if exact:
        assert got.dtype == want.dtype and np.array_equal(got, want), what
    else:
        worst = rel_err(got, want)
        print("%s: largest relative difference %.3e (bound %.3e)" % (what, worst, REL))
        assert got.shape == want.shape and worst <= REL, (what, worst)
        assert np.array_equal(got == 0, want == 0), what


@pytest.mark.parametrize("spacing", EXACT + [ROUNDED])
@pytest.mark.parametrize("shape", SHAPES)
def test_distance_transform_edt_matches_scipy(dev, shape, spacing):
    from scipy.ndimage import distance_transform_edt as scipy_edt
    from cineflow.metrics import distance_transform_edt
    sp = spacing[-len(shape):] if len(shape) == 3 else (spacing[0], spacing[1])          # 2-D: an anisotropic pair, the rounded one included
    for name, m in masks(shape, 11 + len(shape) + shape[-1]):
        want = scipy_edt(m, sampling=sp)
        got = distance_transform_edt(m, sampling=sp)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == shape
        compare(got.cpu().numpy(), want, spacing != ROUNDED, "%s %s %s" % (shape, sp, name))
    # a device tensor, and no sampling, are taken like scipy takes an array
    m = masks(shape, 5)[0][1]
    assert np.array_equal(distance_transform_edt(torch.from_numpy(m).to(dev)).cpu().numpy(), scipy_edt(m))


def test_distance_transform_edt_refuses_a_mask_without_zero(dev):
    from cineflow._lib import CineflowError
    from cineflow.metrics import distance_transform_edt
    with pytest.raises(CineflowError, match="no zero"):
        distance_transform_edt(np.ones((3, 9, 70), np.uint8))
    with pytest.raises(CineflowError, match="no zero"):
        distance_transform_edt(np.ones((9, 70), bool), sampling=(2.0, 0.5))


# ------------------------------------------------------------------------------------------------ surface distances
def blobs(shape, seed, level=0.5):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    f = gaussian_filter(rng.random(shape), 2.0)
    return f > np.quantile(f, level)


def ellipsoid(shape, centre, radii):
    g = np.indices(shape).astype(np.float64)
    return sum(((g[i] - centre[i]) / radii[i]) ** 2 for i in range(len(shape))) <= 1.0


def border_of(mask):
    """medpy: mask ^ binary_erosion(mask, generate_binary_structure(ndim, 1))"""
    from scipy.ndimage import binary_erosion, generate_binary_structure
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, 1), iterations=1)


def surface_cases():
    a, b = blobs((9, 40, 37), 1), blobs((9, 40, 37), 2)
    yield "seeded blobs", a, b
    full_a, full_b = np.ones((9, 40, 37), bool), np.ones((9, 40, 37), bool)
    full_a[4, 20, 18] = False
    full_b[0, 0, 0] = False
    full_b[5:, 30:, :] = False
    yield "touching every face", full_a, full_b
    one, other = np.zeros((9, 40, 37), bool), np.zeros((9, 40, 37), bool)
    one[3, 7, 30] = True
    other[6:8, 20:30, 3:9] = True
    yield "one voxel", one, other
    c1, c2 = np.zeros((9, 40, 37), bool), np.zeros((9, 40, 37), bool)
    c1[:2, :3, :4] = True
    c2[-3:, -2:, -5:] = True
    yield "opposite corners", c1, c2
    yield "2-D pair", blobs((70, 131), 3), blobs((70, 131), 4)
    yield "two offset ellipsoids", ellipsoid((40, 150, 130), (20, 70, 60), (15, 55, 45)), ellipsoid((40, 150, 130), (22, 80, 66), (13, 50, 48))


@pytest.mark.parametrize("case", list(surface_cases()), ids=lambda c: c[0])
def test_surface_distances_edt_has_the_values_of_pairs(dev, case):
    from cineflow.metrics import surface_distances
    name, a, b = case
    for spacing in ((2.5, 0.78125, 0.78125), ROUNDED):
        sp = spacing[-a.ndim:] if a.ndim == 3 else (spacing[0], spacing[1])
        for x, y in ((a, b), (b, a)):
            want = np.sort(surface_distances(x, y, sp, method="pairs").cpu().numpy())
            got = surface_distances(x, y, sp, method="edt")
            assert got.is_cuda and got.dtype == torch.float64
            compare(np.sort(got.cpu().numpy()), want, spacing != ROUNDED, "%s %s" % (name, sp))


@pytest.mark.parametrize("case", list(surface_cases())[:5], ids=lambda c: c[0])
def test_surface_distances_edt_order_is_raster_and_repeats(dev, case):
    from scipy.ndimage import distance_transform_edt as scipy_edt
    from cineflow.metrics import surface_distances
    name, a, b = case
    sp = (2.5, 0.78125, 0.78125)[-a.ndim:]
    want = scipy_edt(~border_of(b), sampling=sp)[border_of(a)]                            # boolean indexing walks the array in raster order
    first = surface_distances(a, b, sp, method="edt").cpu().numpy()
    assert np.array_equal(first, want), name
    assert first.tobytes() == surface_distances(a, b, sp, method="edt").cpu().numpy().tobytes()


def test_surface_distances_edt_empty_masks_raise_like_pairs(dev):
    from cineflow.metrics import surface_distances
    a = blobs((9, 40, 37), 1)
    z = np.zeros_like(a)
    with pytest.raises(RuntimeError, match="first supplied array"):
        surface_distances(z, a, method="edt")
    with pytest.raises(RuntimeError, match="second supplied array"):
        surface_distances(a, z, method="edt")


# ------------------------------------------------------------------------------------------------ the table
def label_volumes():
    rng = np.random.default_rng(7)
    shape = (9, 40, 37)
    f = [blobs(shape, 20 + i, 0.7) for i in range(4)]
    ref = np.zeros(shape, np.uint8)
    for c in (1, 2, 3, 4):
        ref[f[c - 1]] = c
    test = ref.copy()
    flip = rng.random(shape) < 0.08
    test[flip] = rng.integers(0, 5, shape)[flip]
    test = np.roll(test, 1, axis=2)
    return test, ref


class CountingLib:
    """stands in for cineflow's library handle and counts the calls that queue device work (the workspace query is host arithmetic)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("cf_") or name in ("cf_last_error", "cf_edt_workspace_bytes"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def test_label_surface_edt_table_equals_the_per_label_metrics(dev, monkeypatch):
    from cineflow import metrics as M
    test, ref = label_volumes()
    sp = (2.5, 0.78125, 0.78125)
    counter = CountingLib(M.lib())
    monkeypatch.setattr(M, "lib", lambda: counter)
    table = M.label_surface_edt_table(test, ref, [1, 2, 3, 4], sp)
    assert counter.calls == ["cf_label_surface_edt"]                                        # one device call for all labels
    monkeypatch.undo()
    for c in (1, 2, 3, 4):
        t, r = test == c, ref == c
        e = table[c]
        kw = dict(voxel_spacing=sp, method="pairs")
        assert e["hd"] == M.hausdorff_distance(t, r, **kw), c
        assert e["hd95"] == M.hausdorff_distance_95(t, r, **kw), c
        for key, want in (("asd_test_to_ref", M.avg_surface_distance(t, r, reproducible=True, **kw)),
                          ("asd_ref_to_test", M.avg_surface_distance(r, t, reproducible=True, **kw)),
                          ("assd", M.avg_surface_distance_symmetric(t, r, reproducible=True, **kw))):
            print("label %d %s: %.17g vs %.17g" % (c, key, e[key], want))
            assert abs(e[key] - want) <= 1e-15 * want, (c, key, e[key], want)
        assert (e["n_test"], e["n_ref"]) == (int(border_of(t).sum()), int(border_of(r).sum()))
        assert np.array_equal(np.sort(e["d_test_to_ref"]), np.sort(M.surface_distances(t, r, sp, method="pairs").cpu().numpy()))
        assert np.array_equal(np.sort(e["d_ref_to_test"]), np.sort(M.surface_distances(r, t, sp, method="pairs").cpu().numpy()))
    again = M.label_surface_edt_table(test, ref, [1, 2, 3, 4], sp)
    for c in (1, 2, 3, 4):
        for key in ("d_test_to_ref", "d_ref_to_test"):
            assert table[c][key].tobytes() == again[c][key].tobytes()
        assert all(table[c][k] == again[c][k] for k in ("hd", "hd95", "asd_test_to_ref", "asd_ref_to_test", "assd"))


def test_label_surface_edt_table_absent_and_full_labels_are_nan(dev):
    from cineflow.metrics import label_surface_edt_table
    test, ref = label_volumes()
    test = test.copy()
    test[test == 3] = 0                                                                      # label 3 only in the reference, label 9 nowhere
    table = label_surface_edt_table(test, ref, [1, 3, 9, 2], (1.0, 1.0, 1.0))
    for c in (3, 9):
        e = table[c]
        assert e["d_test_to_ref"].size == 0 and e["d_ref_to_test"].size == 0
        assert all(np.isnan(e[k]) for k in ("hd", "hd95", "asd_test_to_ref", "asd_ref_to_test", "assd"))
    assert table[3]["n_ref"] > 0 and table[3]["n_test"] == 0
    assert table[1]["hd"] > 0 and table[2]["hd"] > 0 and table[2]["d_ref_to_test"].size == table[2]["n_ref"]
    full = label_surface_edt_table(np.ones((4, 6, 5), np.uint8), np.ones((4, 6, 5), np.uint8), [1])[1]
    assert np.isnan(full["hd"]) and full["d_test_to_ref"].size == 0 and full["n_test"] == 4 * 6 * 5 - 2 * 4 * 3


# ------------------------------------------------------------------------------------------------ surface Dice
def test_normalized_surface_dice_matches_the_formula_on_scipy_distances(dev):
    from scipy.ndimage import distance_transform_edt as scipy_edt
    from cineflow.metrics import normalized_surface_dice
    a, b = blobs((9, 40, 37), 1), blobs((9, 40, 37), 2)
    sp = (2.5, 0.78125, 0.78125)
    a_to_b = scipy_edt(~border_of(b), sampling=sp)[border_of(a)]
    b_to_a = scipy_edt(~border_of(a), sampling=sp)[border_of(b)]
    positive = np.sort(a_to_b[a_to_b > 0])
    at_a_distance = float(positive[positive.size // 3])
    for threshold in (0, 1.0, at_a_distance):
        tp_a, tp_b = np.sum(a_to_b <= threshold) / len(a_to_b), np.sum(b_to_a <= threshold) / len(b_to_a)
        fp, fn = np.sum(a_to_b > threshold) / len(a_to_b), np.sum(b_to_a > threshold) / len(b_to_a)
        want = (tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8)
        for method in (None, "pairs", "edt"):
            assert normalized_surface_dice(a, b, threshold, sp, method=method) == want, (threshold, method)
