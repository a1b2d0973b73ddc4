"""cf_cc_label / cf_cc_sizes (csrc/cc_label.hip) on the device.

cf_cc_label must equal scipy.ndimage.label as a partition -- stated here as "1 + the smallest flat index of the scipy component", which pins
the label values too -- and the converged cf_cc_init / cf_cc_sweep labels bit for bit.  Shapes are the smallest at which the tiled union-find
(tiles of 4 x 8 x 32 voxels) can go wrong: one voxel, nothing to label, sizes that are no multiple of any tile edge, one component crossing
every tile boundary many times, a path around tile corners, ties, contact with all six faces, diagonal-only contact, every voxel a component
of its own (the fullest size hash table), label values up to 255; each in both region_of modes.  Every comparison is exact.  Expected labels
are computed once per case on the CPU, shared and write-protected."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def draw_path(img, points, value=1):
    """fill the axis-aligned segments between successive points (z, then y, then x moves): a face-connected path"""
    cur = list(points[0])
    img[tuple(cur)] = value
    for p in points[1:]:
        for ax in range(3):
            while cur[ax] != p[ax]:
                cur[ax] += 1 if p[ax] > cur[ax] else -1
                img[tuple(cur)] = value
    return img


def build(name):
    rng = np.random.default_rng(7)
    if name == "one_voxel":
        return np.ones((1, 1, 1), np.uint8)
    if name == "empty":
        return np.zeros((3, 9, 40), np.uint8)
    if name == "flat_130x70":
        return ((rng.random((1, 130, 70)) < 0.6) * rng.integers(1, 4, (1, 130, 70))).astype(np.uint8)
    if name == "odd_5x37x43":
        return ((rng.random((5, 37, 43)) < 0.55) * rng.integers(1, 4, (5, 37, 43))).astype(np.uint8)
    if name == "serpentine":                                    # one component, every row joined to the next at alternating ends
        img = np.zeros((1, 64, 64), np.uint8)
        for y in range(0, 64, 2):
            img[0, y, :] = 1
            if y + 1 < 64:
                img[0, y + 1, 63 if (y // 2) % 2 == 0 else 0] = 1
        return img
    if name == "helix":                                         # winds round the tile corner at (z, y, x) = (4, 8, 32) and the next ones
        img = np.zeros((10, 18, 68), np.uint8)
        pts = []
        for turn in range(4):
            z = 1 + 2 * turn
            pts += [(z, 6, 30), (z, 6, 34), (z + 1, 10, 34), (z + 1, 10, 30)]
        draw_path(img, pts, 2)
        draw_path(img, [(0, 16, 0), (0, 16, 67), (9, 16, 67)], 3)
        return img
    if name == "tie":                                           # two components of 24 voxels each, and a smaller one
        img = np.zeros((4, 12, 40), np.uint8)
        img[0:2, 1:4, 2:6] = 1
        img[2:4, 8:11, 30:34] = 1
        img[1, 6, 20:23] = 1
        return img
    if name == "six_faces":                                     # three bars through the centre reach all six faces
        img = np.zeros((6, 20, 70), np.uint8)
        img[:, 10, 35] = 1
        img[3, :, 35] = 1
        img[3, 10, :] = 1
        img[0, 0, 0] = 1
        return img
    if name == "checkerboard":                                  # diagonal contact only: every set voxel is a component of its own
        z, y, x = np.indices((5, 37, 43))
        return ((z + y + x) % 2).astype(np.uint8)
    if name == "alternating":                                   # classes 1 and 2 alternate: one joint object, n singletons per class
        z, y, x = np.indices((4, 16, 64))
        return (1 + (z + y + x) % 2).astype(np.uint8)
    if name == "values_to_255":
        vals = np.array([0, 7, 100, 200, 255], np.uint8)
        return vals[rng.integers(0, 5, (3, 21, 45))]
    raise KeyError(name)


CASES = ("one_voxel", "empty", "flat_130x70", "odd_5x37x43", "serpentine", "helix", "tie", "six_faces", "checkerboard", "alternating",
         "values_to_255")
MODES = ("joint", "own")


def region_table(mode):
    tab = np.zeros(256, np.uint8)
    tab[1:] = 1 if mode == "joint" else np.arange(1, 256)
    return tab


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """(image, labels int32) with labels = 1 + smallest flat index of the scipy.ndimage.label component of the voxel's region"""
    from scipy.ndimage import label
    img = build(name)
    reg = region_table(mode)[img]
    out = np.zeros(img.shape, np.int32)
    flat = np.arange(img.size, dtype=np.int64).reshape(img.shape)
    for r in np.unique(reg[reg > 0]):
        lmap, k = label(reg == r)
        if k:
            first = np.full(k + 1, img.size, np.int64)
            np.minimum.at(first, lmap.reshape(-1), flat.reshape(-1))
            out[lmap > 0] = (first[lmap[lmap > 0]] + 1).astype(np.int32)
    img.setflags(write=False)
    out.setflags(write=False)
    return img, out


def device_labels(dev, img, mode):
    from cineflow import ops
    return ops.connected_component_labels(torch.from_numpy(np.array(img)).to(dev), region_table(mode).tolist())


def sweep_labels(dev, img, mode):
    """the old route: cf_cc_init + cf_cc_sweep to convergence, one region at a time"""
    from cineflow import ops
    from cineflow._lib import check, lib
    regions = [(1,)] if mode == "joint" else [(int(v),) for v in np.unique(img) if v]
    src = (img > 0).astype(np.uint8) if mode == "joint" else img
    t = torch.from_numpy(np.array(src)).to(dev)
    D, H, W = img.shape
    out = torch.zeros(img.size, dtype=torch.int32, device=dev)
    labels = torch.empty(img.size, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for vals in regions:
        cls = (ctypes.c_uint8 * len(vals))(*vals)
        check(lib().cf_cc_init(t.data_ptr(), labels.data_ptr(), img.size, ctypes.cast(cls, ctypes.c_void_p), len(vals), ops._stream()), "cf_cc_init")
        for _ in range(10000):
            changed.zero_()
            for _ in range(16):
                check(lib().cf_cc_sweep(labels.data_ptr(), D, H, W, changed.data_ptr(), ops._stream()), "cf_cc_sweep")
            if int(changed.item()) == 0:
                break
        else:
            raise AssertionError("cf_cc_sweep did not converge")
        out += labels
    return out.reshape(img.shape)


def test_the_cases_hold_what_they_are_there_for():
    """CPU only: the fixtures really have the properties the GPU tests lean on."""
    from scipy.ndimage import label
    assert label(build("serpentine"))[1] == 1 and label(build("helix") == 2)[1] == 1 and label(build("six_faces"))[1] == 2
    img = build("six_faces")
    big = label(img)[0] == label(img)[0][3, 10, 35]
    assert big[0].any() and big[-1].any() and big[:, 0].any() and big[:, -1].any() and big[:, :, 0].any() and big[:, :, -1].any()
    sizes = np.bincount(label(build("tie"))[0].reshape(-1))[1:]
    assert sorted(sizes.tolist()) == [3, 24, 24]
    cb = build("checkerboard")
    assert label(cb)[1] == int(cb.sum())
    assert label(build("alternating") > 0)[1] == 1 and label(build("alternating") == 1)[1] == build("alternating").size // 2
    assert build("values_to_255").max() == 255
    helix = np.argwhere(build("helix") == 2)                    # the path really passes tile corners: it has voxels in >= 8 tiles
    assert len({(z // 4, y // 8, x // 32) for z, y, x in helix}) >= 8


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_labels_equal_scipy_and_the_converged_sweeps(dev, name, mode):
    img, want = expected(name, mode)
    got = device_labels(dev, img, mode)
    assert got.dtype == torch.int32 and tuple(got.shape) == img.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "%d of %d labels differ from scipy.ndimage.label" % (int((got != want).sum()), want.size)
    old = sweep_labels(dev, img, mode).cpu().numpy()
    assert np.array_equal(got, old), "%d of %d labels differ from cf_cc_init + cf_cc_sweep" % (int((got != old).sum()), want.size)


def test_a_region_table_that_names_nothing_labels_nothing(dev):
    from cineflow import ops
    img, _ = expected("odd_5x37x43", "own")
    got = ops.connected_component_labels(torch.from_numpy(np.array(img)).to(dev), {9: 1})
    assert int(got.abs().sum().item()) == 0
    two_d = ops.connected_component_labels(torch.from_numpy(np.array(img[0])).to(dev), {1: 1, 2: 1, 3: 1})
    assert tuple(two_d.shape) == img.shape[1:]
    assert np.array_equal(two_d.cpu().numpy(), expected_2d(img[0]))


def expected_2d(img2):
    from scipy.ndimage import label
    lmap, k = label(img2 > 0)
    flat = np.arange(img2.size).reshape(img2.shape)
    out = np.zeros(img2.shape, np.int32)
    for o in range(1, k + 1):
        out[lmap == o] = flat[lmap == o].min() + 1
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_sizes_equal_bincount(dev, name, mode):
    from cineflow import ops
    img, want = expected(name, mode)
    tab = region_table(mode)
    t = torch.from_numpy(np.array(img)).to(dev)
    labels = torch.from_numpy(np.array(want)).to(dev)
    counts, region_max = ops.connected_component_sizes(labels.reshape(-1), t, tab.tolist())
    want_counts = np.bincount(want.reshape(-1), minlength=img.size + 1)[1:].astype(np.int32)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    want_max = np.zeros(256, np.int32)
    roots = np.flatnonzero(want_counts)
    np.maximum.at(want_max, tab[img.reshape(-1)[roots]], want_counts[roots])
    assert np.array_equal(region_max.cpu().numpy(), want_max)
    # alive: whole components, every other one by the parity of its root index
    alive = ((want % 4) < 2) & (want > 0)
    counts2, region_max2, region_max_alive = ops.connected_component_sizes(labels.reshape(-1), t, tab.tolist(),
                                                                           alive=torch.from_numpy(alive.astype(np.uint8)).to(dev))
    want_alive = np.zeros(256, np.int32)
    live = roots[((roots + 1) % 4) < 2]
    np.maximum.at(want_alive, tab[img.reshape(-1)[live]], want_counts[live])
    assert np.array_equal(counts2.cpu().numpy(), want_counts) and np.array_equal(region_max2.cpu().numpy(), want_max)
    assert np.array_equal(region_max_alive.cpu().numpy(), want_alive)


def test_the_tie_keeps_both_largest_components(dev):
    """sizes that equal the maximum stay (connected_components.py:95): after cf_cc_apply only the 3-voxel object is gone"""
    from cineflow import ops
    img, want = expected("tie", "joint")
    t = torch.from_numpy(np.array(img)).to(dev)
    labels = device_labels(dev, img, "joint")
    counts, mx = ops.connected_component_sizes(labels.reshape(-1), t, region_table("joint").tolist())
    assert int(mx[1].item()) == 24
    out = ops.cc_apply(t, 2, True, [], labels, counts, mx, None, None, None, 1.0).cpu().numpy()
    assert int(out.sum()) == 48 and out[1, 6, 20:23].sum() == 0
