"""Operator-level tables for csrc/preprocess.hip (and cf_cc_init / cf_cc_sweep as the hole fill uses them): every kernel against the plain
restatements of tests/_kernel_refs.py (pinned to the oracle in test_kernel_refs_cpu.py), at the sizes where a flat launch takes its second
grid-stride trip (n > 2^20 for one element per thread, n > 2^24 for the 16-per-thread reductions), at one element, around a block, and on
the values where the semantics live (NaN, -0.0, denormals, infinities, the clip ends, strict range ends).

Bars.  Masks, boxes, labels, counts, min / max: identical.  cf_normalize, cf_slab_clip_to_f32, cf_nan_to_zero, cf_assign_where_ge: bit
for bit (correctly rounded IEEE operations on both sides).  cf_masked_moments: the count exact, each sum within n * 2^-53 * sum|term| of
numpy's fp64 sum of the same fp32 values (the worst case of an fp64 sum in any order).  cf_spline3_resample_axis: 1e-12 x max|x| of the
line against scipy.ndimage.zoom (the kernel claims 1e-14 relative for its 24-tap truncation of the prefilter; 52 taps whose coefficient
magnitudes sum to under 3 add fp64 rounding far below that; two orders of margin).

One finding.  cf_normalize clipped with fminf(fmaxf(x, lo), hi), which turns a NaN into lo where np.clip keeps it (PreprocessorFor2D
does not remove NaNs before a CT scheme): the clip rows of test_normalize_table missed "NaN positions equal" at both NaN inputs (index 8
and n - 5) until the kernel left NaN alone.  crop_to_nonzero with a created segmentation and a positive nonzero_label now gives the
all-zero map the reference's `[> 0] = 0` leaves (the device wrote the label outside the mask).

Measured on the MI355X (pytest -s prints one line per row: worst figure, bar, ratio):
  masks (14 rows), boxes, cf_seg_outside_mask, cf_normalize (30 rows), cf_nan_to_zero, cf_assign_where_ge, slab min / max / clip (32 rows):
      0 differing values; the 128 x 128 spiral takes 33-34 rounds of 8 sweeps
  cf_masked_moments (25 rows): counts exact; sum <= 0.001 of its bar, sum of squares <= 0.008 (n = 257, range);
      at n = 16,840,265: |sum - numpy| 3.8e-6 against a bar of 13, |sum of squares - numpy| 3.9e-3 against 5.4e3
  cf_spline3_resample_axis (33 rows): worst 1.80e-14 x max|x| (3 x 25 x 1500 -> 250), ratio 0.018; no row exceeds 1e-13 x max|x|
"""
import ctypes

import numpy as np
import pytest
import torch

from _kernel_refs import bbox as ref_bbox
from _kernel_refs import cubic_axis, masked_moments, nonzero_fill_holes, normalize_f32, ratio_line, seg_outside_mask, slab_clip_f32, slab_minmax

pytestmark = pytest.mark.gpu

BIG = (17, 251, 247)                  # 1,053,949 voxels: the second trip of a 4096 x 256 one-per-thread launch covers the last 5,373
N20 = 17 * 251 * 247
N24 = 65 * 509 * 509                  # 16,840,265 > 2^24: the second trip of the 16-per-thread reductions


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(got, want):
    """bit-identical except that NaN only has to sit where NaN sits"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ at %s" % (np.nonzero(np.isnan(got) != nan)[0][:8],)
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), "%d values differ, first at %s: got %r want %r" % (bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


# ------------------------------------------------------------------------------------------------ create_nonzero_mask + fill holes
def _hollow(shape, lo, hi):
    """a solid box lo..hi (exclusive) with its interior carved out"""
    m = np.zeros(shape, np.float32)
    m[tuple(slice(a, b) for a, b in zip(lo, hi))] = 1
    m[tuple(slice(a + 1, b - 1) for a, b in zip(lo, hi))] = 0
    return m


def _spiral(n, open_end):
    """n x n foreground with a one-pixel background corridor spiralling from the centre outwards; open_end carries it to the border"""
    m = np.ones((n, n), np.float32)
    y = x = n // 2
    dy, dx, run = 0, 1, 2
    while True:
        for _ in range(2):
            for _ in range(run):
                if not (1 <= y < n - 1 and 1 <= x < n - 1):
                    if open_end:
                        m[min(max(y, 0), n - 1), min(max(x, 0), n - 1)] = 0
                    return m
                m[y, x] = 0
                y, x = y + dy, x + dx
            dy, dx = dx, -dy
        run += 2


def _blobs(shape, seed, nblob):
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.float32)
    for b in range(nblob):
        size = [int(rng.integers(3, max(4, min(s // 2, 40)))) for s in shape]
        lo = [int(rng.integers(0, s - z + 1)) for s, z in zip(shape, size)]
        hi = [a + z for a, z in zip(lo, size)]
        m[tuple(slice(a, c) for a, c in zip(lo, hi))] = rng.normal() + 3.0
        if b % 3 == 0 and all(z >= 3 for z in size):        # an enclosed hole (unless a later blob or the array face opens it)
            m[tuple(slice(a + 1, c - 1) for a, c in zip(lo, hi))] = 0
    return m


def mask_cases():
    c = {}
    base = _hollow((6, 20, 18), (1, 3, 2), (5, 15, 14))
    base[2, 8, 8] = 1                                                  # an island inside the cavity
    c["C1 cavity"] = base[None]
    nan2 = np.stack([base, -0.0 * np.ones_like(base)])                 # -0.0 is zero ...
    nan2[1, 0, 0, 0] = np.nan                                          # ... and NaN is not
    c["C2 NaN / -0.0"] = nan2
    c3 = np.stack([base * 0, -0.0 * np.ones_like(base), base])
    c3[0, 3, 9, 9] = np.nan                                            # a NaN voxel inside the cavity is foreground
    c["C3 NaN inside the cavity"] = c3
    ring = _hollow((9, 11), (2, 2), (7, 9))
    c["one slice as (C, 1, H, W): nothing fills"] = np.stack([ring, ring * 0])[:, None]
    c["the same slice as (C, H, W): fills"] = np.stack([ring, ring * 0])
    shaft = np.ones((4, 9, 9), np.float32)
    shaft[0:2, 3:6, 3:6] = 0
    c["cavity open at z = 0: stays"] = shaft[None]
    deep = np.ones((4, 9, 9), np.float32)
    deep[1:3, 3:6, 3:6] = 0
    c["cavity one plane deeper: fills"] = deep[None]
    far = np.ones((4, 9, 9), np.float32)
    far[2:4, 3:6, 3:6] = 0
    c["cavity open at z = D - 1: stays"] = far[None]
    diag = np.ones((6, 6), np.float32)
    for i in range(4):
        diag[i, i] = 0
    c["2-D diagonal chain to the corner: fills"] = diag[None]
    d3 = np.ones((3, 6, 6), np.float32)
    d3[1] = diag
    c["3-D diagonal chain to an edge: fills"] = d3[None]
    c["spiral corridor, enclosed"] = _spiral(128, False)[None]
    c["spiral corridor, open at the border"] = _spiral(128, True)[None]
    big = _blobs(BIG, 7, 160)
    big[16, 236:246, 200:240] = 2.0                                    # in the last 5,000 voxels: closed in-plane, open at the z face
    big[16, 238:244, 205:235] = 0
    big[8:13, 100:120, 100:130] = 1.5                                  # an enclosed 3-D hole in the first trip
    big[9:12, 102:118, 102:128] = 0
    c["17 x 251 x 247 blobs (> 2^20)"] = big[None]
    flat = _blobs((1031, 1021), 8, 200)                                # 1,052,651 pixels as 2-D data: holes fill in the second trip too
    flat[1021:1031, 900:1000] = 4.0
    flat[1023:1030, 905:995] = 0
    c["1031 x 1021 blobs as 2-D (> 2^20)"] = flat[None]
    return c


@pytest.fixture(scope="module")
def mask_table():
    return {k: (v, nonzero_fill_holes(v)) for k, v in mask_cases().items()}


def test_create_nonzero_mask_table(dev, mask_table):
    from cineflow import preprocessing as P
    print()
    for tag, (data, want) in mask_table.items():
        got = P.create_nonzero_mask(data)
        assert got.dtype == bool and got.shape == want.shape, tag
        ratio_line("nonzero mask: " + tag, float((got != want).sum()), 0)
        assert np.array_equal(got, want), "%s: %d voxels differ" % (tag, (got != want).sum())
    # the rows mean what their names say
    t = mask_table
    raw = lambda k: np.any(t[k][0] != 0, 0)                                                    # noqa: E731
    assert np.array_equal(t["one slice as (C, 1, H, W): nothing fills"][1], raw("one slice as (C, 1, H, W): nothing fills"))
    assert t["the same slice as (C, H, W): fills"][1].sum() == raw("the same slice as (C, H, W): fills").sum() + 15
    assert np.array_equal(t["cavity open at z = 0: stays"][1], raw("cavity open at z = 0: stays")) and t["cavity one plane deeper: fills"][1].all()
    assert np.array_equal(t["cavity open at z = D - 1: stays"][1], raw("cavity open at z = D - 1: stays"))
    assert t["2-D diagonal chain to the corner: fills"][1].sum() == 35 and t["3-D diagonal chain to an edge: fills"][1].sum() == 107
    assert t["spiral corridor, enclosed"][1].all() and np.array_equal(t["spiral corridor, open at the border"][1], raw("spiral corridor, open at the border"))
    assert t["C2 NaN / -0.0"][1][0, 0, 0] and not t["C2 NaN / -0.0"][1][0, 0, 1] and t["C3 NaN inside the cavity"][1].sum() == t["C1 cavity"][1].sum()
    for k in ("17 x 251 x 247 blobs (> 2^20)", "1031 x 1021 blobs as 2-D (> 2^20)"):
        assert t[k][1].sum() > raw(k).sum() + 500, k                                           # holes were filled ...
    assert not t["17 x 251 x 247 blobs (> 2^20)"][1][16, 240, 220] and t["1031 x 1021 blobs as 2-D (> 2^20)"][1][1029, 950]   # ... and the last-5,000 pockets decided


def test_spiral_needs_more_than_one_round_of_sweeps(dev):
    """the corridor's labels travel further than 8 sweeps carry them: the wrapper's `changed` loop is what the spiral rows test"""
    from cineflow._lib import check, lib
    m = torch.from_numpy((_spiral(128, False) != 0).astype(np.uint8)).to(dev).reshape(-1)
    labels = torch.empty(m.numel(), dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    zero = (ctypes.c_uint8 * 1)(0)
    check(lib().cf_cc_init(m.data_ptr(), labels.data_ptr(), m.numel(), ctypes.cast(zero, ctypes.c_void_p), 1, _stream()), "cf_cc_init")
    rounds = 0
    while rounds < 4096:
        changed.zero_()
        for _ in range(8):
            check(lib().cf_cc_sweep(labels.data_ptr(), 1, 128, 128, changed.data_ptr(), _stream()), "cf_cc_sweep")
        rounds += 1
        if int(changed.item()) == 0:
            break
    print("\n  spiral 128 x 128: %d rounds of 8 sweeps" % rounds)
    assert 2 < rounds < 4096
    lab = labels.cpu().numpy()
    assert len(np.unique(lab[lab != 0])) == 1 and (lab != 0).sum() == (_spiral(128, False) == 0).sum()


# ------------------------------------------------------------------------------------------------ get_bbox_from_mask
def test_bbox_table(dev):
    from cineflow import preprocessing as P
    D, H, W = 5, 7, 6
    for z in (0, D - 1):
        for y in (0, H - 1):
            for x in (0, W - 1):
                m = np.zeros((D, H, W), np.uint8)
                m[z, y, x] = 1
                assert P.get_bbox_from_mask(m) == ref_bbox(m) == [[z, z + 1], [y, y + 1], [x, x + 1]]
    assert P.get_bbox_from_mask(np.ones((D, H, W), np.uint8)) == [[0, D], [0, H], [0, W]]
    m = np.zeros((D, H, W), np.float32)
    m[1, 2, 3] = m[3, 5, 1] = -2.5                                     # outside_value: everything that differs from it counts
    assert P.get_bbox_from_mask(m) == ref_bbox(m) == [[1, 4], [2, 6], [1, 4]]
    assert P.get_bbox_from_mask(m, outside_value=-2.5) == [[0, D], [0, H], [0, W]]
    with pytest.raises(ValueError):
        P.get_bbox_from_mask(np.zeros((D, H, W), np.uint8))
    with pytest.raises(ValueError):
        ref_bbox(np.zeros((D, H, W), np.uint8))
    big = torch.zeros((65, 509, 509), dtype=torch.uint8)               # 16,840,265 voxels: only the second trip sees the last plane
    big[64, 508, 300] = 1
    big[64, 200, 508] = 1
    big[0, 0, 5] = 1
    assert P.get_bbox_from_mask(big.to(dev)) == [[0, 65], [0, 509], [5, 509]]
    big[0, 0, 5] = 0
    assert P.get_bbox_from_mask(big.to(dev)) == [[64, 65], [200, 509], [300, 509]]


# ------------------------------------------------------------------------------------------------ crop_to_nonzero / cf_seg_outside_mask
@pytest.mark.parametrize("label", [-1, 5])
def test_crop_to_nonzero_given_seg(dev, label):
    from cineflow import preprocessing as P
    from oracle import preprocess as OP
    rng = np.random.default_rng(11)
    data = np.zeros((2, 7, 15, 13), np.float32)
    data[0, 1:6, 2:12, 3:11] = rng.normal(size=(5, 10, 8))
    data[0, 2:5, 4:9, 5:9] = 0                                         # a filled cavity ...
    data[1, 1:6, 2:4, 3:5] = 0
    data[0, 1:6, 2:4, 3:5] = 0                                         # ... and a corner notch that stays outside the mask
    seg = rng.choice(np.array([0.0, -0.0, 3.0], np.float32), size=(2,) + data.shape[1:])
    seg[1] = np.roll(seg[0], 1, axis=2)                                # two channels that differ: the mask is indexed by i % V
    d0, s0, b0 = OP.crop_to_nonzero(data.copy(), seg.copy(), label)
    d1, s1, b1 = P.crop_to_nonzero(data.copy(), seg.copy(), label)
    assert b1 == b0 and np.array_equal(d1, d0)
    assert s1.dtype == seg.dtype and np.array_equal(s1, s0)
    sl = (slice(None),) + tuple(slice(*b) for b in b0)
    mask = nonzero_fill_holes(data)[sl[1:]]
    assert np.array_equal(s1, seg_outside_mask(seg[sl], mask, label))
    assert (s1 == label).sum() == 2 * (mask == 0).sum() - (seg[sl] == 3)[:, mask == 0].sum() and (mask == 0).any()
    assert np.array_equal(_bits(s1)[:, mask], _bits(seg[sl])[:, mask])  # inside the mask nothing is touched, -0.0 included
    d2, s2, b2 = P.crop_to_nonzero(data.copy(), None, label)           # the created segmentation (all zero for a positive label, as in the reference)
    _, s3, _ = OP.crop_to_nonzero(data.copy(), None, label)
    assert b2 == b0 and s2.shape == s3.shape and np.array_equal(s2, s3) and (s3 == label).any() == (label < 0)


# ------------------------------------------------------------------------------------------------ _moments
def _raw_moments(dev, x, seg, lo, hi):
    from cineflow._lib import check, lib
    xd = torch.from_numpy(x).to(dev)
    sd = None if seg is None else torch.from_numpy(seg).to(dev)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    check(lib().cf_masked_moments(xd.data_ptr(), None if sd is None else sd.data_ptr(), x.size, int(lo is not None), float(lo or 0.0), float(hi or 0.0),
                                  out.data_ptr(), _stream()), "cf_masked_moments")
    return out.cpu().tolist(), xd, sd


@pytest.fixture(scope="module")
def moment_values():
    rng = np.random.default_rng(21)
    return (400.0 + 100.0 * rng.standard_normal(N24)).astype(np.float32), rng.integers(-1, 3, N24).astype(np.float32)


@pytest.mark.parametrize("n", [1, 255, 257, N20, N24])
def test_masked_moments_table(dev, moment_values, n):
    """the n = 16,840,265 row is the cancellation-prone one of the issue: 400 + 100 N(0, 1), whose variance is s2 / n - mean^2"""
    from cineflow import preprocessing as P
    vals, segs = moment_values
    x, seg = vals[N24 - n:], segs[N24 - n:]                            # the tail: every n ends on the same last values
    lo, hi = np.float32(350.0), np.float32(462.5)
    xr = x.copy()
    xr[:: max(n // 7, 1)] = lo                                         # values exactly at the ends are excluded (strict inequalities)
    xr[-1] = hi
    print()
    for tag, xx, sg, a, b in (("plain", x, None, None, None), ("seg", x, seg, None, None), ("range", xr, None, lo, hi), ("seg + range", xr, seg, lo, hi),
                              ("all-negative seg", x, -np.ones_like(x), None, None)):
        cnt, r1, r2, ra = masked_moments(xx, sg, a, b)
        (s1, s2, c), xd, sd = _raw_moments(dev, xx, sg, a, b)
        assert c == cnt, "%s n=%d: count %r != %d" % (tag, n, c, cnt)
        b1, b2 = n * 2.0 ** -53 * ra, n * 2.0 ** -53 * r2
        ratio_line("moments n=%d %s: sum" % (n, tag), abs(s1 - r1), b1)
        ratio_line("moments n=%d %s: sum of squares" % (n, tag), abs(s2 - r2), b2)
        assert abs(s1 - r1) <= b1 and abs(s2 - r2) <= b2, (tag, n, s1, r1, s2, r2)
        mean, sd_ = P._moments(xd, sd, a, b)
        if cnt == 0:
            assert np.isnan(mean) and np.isnan(sd_) and s1 == 0 and s2 == 0
        else:
            assert abs(mean - r1 / cnt) <= b1 / cnt + 2.0 ** -52 * abs(r1 / cnt)
    if 1 < n <= N20:
        assert masked_moments(xr, None, lo, hi)[0] < masked_moments(xr, None, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf))[0]


# ------------------------------------------------------------------------------------------------ _normalize / cf_nan_to_zero / cf_assign_where_ge
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, np.inf, -np.inf, np.nan, -2.0, 2.0, 3.4028235e38, -3.4028235e38], np.float32)


def _normalize_input(n, lo, hi):
    rng = np.random.default_rng(n)
    x = (3.0 * rng.standard_normal(n)).astype(np.float32)
    sp = np.concatenate([SPECIALS, [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf)]]).astype(np.float32)
    k = min(len(sp), n)
    x[:k] = sp[:k]
    if n > 2 * len(sp):
        x[-len(sp):] = sp                                              # and in the second grid-stride trip
    return x


@pytest.mark.parametrize("n", [1, 19, (1 << 20) - 1, (1 << 20) + 1, N20])
def test_normalize_table(dev, n):
    from cineflow import preprocessing as P
    lo, hi = np.float32(-2.0), np.float32(2.0)
    x = _normalize_input(n, lo, hi)
    seg = np.random.default_rng(n + 1).choice(np.array([-1.0, 0.0, 2.0], np.float32), size=n)
    print()
    for tag, sub, div, clip, zo in (("plain", 0.3, 1.7, None, False), ("clip", 0.3, 1.7, (lo, hi), False), ("clip + zero outside", -0.41, 0.013, (lo, hi), True),
                                    ("zero outside", 0.3, 1.7, None, True), ("denormal quotients", 0.0, 3.0, None, False),
                                    ("float32 scalars", np.float32(0.1), np.float32(0.7) + np.float32(1e-8), None, False)):
        want = normalize_f32(x, sub, div, clip, seg, zo)
        xd = torch.from_numpy(x.copy()).to(dev)
        P._normalize(xd, torch.from_numpy(seg).to(dev) if zo else None, sub, div, clip=clip, zero_outside=zo)
        got = xd.cpu().numpy()
        ratio_line("normalize n=%d %s: differing values" % (n, tag), float(((_bits(got) != _bits(want)) & ~np.isnan(want)).sum()), 0)
        same_bits(got, want)


@pytest.mark.parametrize("n", [1, 19, N20])
def test_nan_to_zero_and_assign_where_ge(dev, n):
    from cineflow._lib import check, lib
    x = _normalize_input(n, np.float32(-2.0), np.float32(2.0))
    x[::5] = np.nan
    want = np.where(np.isnan(x), np.float32(0), x)
    xd = torch.from_numpy(x.copy()).to(dev)
    check(lib().cf_nan_to_zero(xd.data_ptr(), n, _stream()), "cf_nan_to_zero")
    got = xd.cpu().numpy()
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want))          # +-inf, -0.0 and denormals bit-identical
    src = np.random.default_rng(n).random(n).astype(np.float32)
    edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, np.nextafter(np.float32(0.5), np.float32(1)), np.inf, -np.inf, 0.0], np.float32)
    k = min(n, len(edge))
    src[:k] = edge[:k]
    if n > 2 * len(edge):
        src[-len(edge):] = edge
    dst = np.random.default_rng(n + 1).normal(size=n).astype(np.float32)
    want = np.where(src >= np.float32(0.5), np.float32(7.0), dst)                       # NaN >= 0.5 is false: not assigned
    dd, sd = torch.from_numpy(dst.copy()).to(dev), torch.from_numpy(src).to(dev)
    check(lib().cf_assign_where_ge(dd.data_ptr(), sd.data_ptr(), n, 0.5, 7.0, _stream()), "cf_assign_where_ge")
    assert np.array_equal(_bits(dd.cpu().numpy()), _bits(want))
    if n >= len(edge):
        assert want[0] == 7.0 and want[1] == dst[1] and want[2] == dst[2] and want[3] == 7.0


# ------------------------------------------------------------------------------------------------ cf_spline3_resample_axis
def _spline_ms(n):
    return sorted({1, 10 * n, int(round(1.37 * n)) + 1, max(1, int(round(0.61 * n))), 3 * n + 1} - {n})


def _spline_row(dev, outer, n, inner, m, seed):
    from cineflow import preprocessing as P
    x = np.random.default_rng(seed).normal(size=(outer, n, inner)) * 50.0 + 300.0
    want = cubic_axis(x, 1, m)
    got = P._spline_axis(torch.from_numpy(x).to(dev), 1, m).cpu().numpy()
    assert got.shape == want.shape == (outer, m, inner) and got.dtype == np.float64
    return float((np.abs(got - want) / np.abs(x).max(axis=1, keepdims=True)).max())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 25, 236])
def test_spline_axis_table(dev, n):
    print()
    for m in _spline_ms(n):
        worst = max(_spline_row(dev, outer, n, inner, m, 1000 * n + m) for outer in (1, 3) for inner in (1, 7))
        ratio_line("spline n=%d -> m=%d (outer 1 / 3, inner 1 / 7)" % (n, m), worst, 1e-12)
        assert worst <= 1e-12, (n, m, worst)


def test_spline_axis_second_trip(dev):
    outer, n, inner, m = 3, 25, 1500, 250                              # 1,125,000 outputs
    worst = _spline_row(dev, outer, n, inner, m, 5)
    print()
    ratio_line("spline 3 x 25 x 1500 -> m=250 (> 2^20 outputs)", worst, 1e-12)
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------ cf_slab_minmax / cf_slab_clip_to_f32
@pytest.mark.parametrize("A,B", [(23, 89), (1, 2047), (8, 256), (1, 2048), (3, 683), (1, 2049), (3, 43691), (1, 64 * 2048 + 1)])
def test_slab_minmax_and_clip(dev, A, B):
    from cineflow._lib import check, lib
    print()
    for C in (1, 2):
        for S in (1, 5):
            rng = np.random.default_rng(A * B + C + S)
            x = rng.normal(size=(C, A, S, B)) * 40.0 + 100.0
            x[C - 1, A - 1, S - 1, B - 1] = 1e4                        # extrema in the last element and the first
            x[0, 0, 0, 0] = -1e4
            mn, mx = slab_minmax(x)
            nchunk = lib().cf_slab_minmax_chunks(C, A, S, B)
            assert nchunk == min(max((A * B + 2047) // 2048, 1), 64)
            xd = torch.from_numpy(x).to(dev)
            mm = torch.full((C * S * 2,), float("nan"), dtype=torch.float64, device=dev)
            part = torch.full((C * S * 2 * nchunk,), float("nan"), dtype=torch.float64, device=dev)
            check(lib().cf_slab_minmax(xd.data_ptr(), C, A, S, B, mm.data_ptr(), part.data_ptr(), _stream()), "cf_slab_minmax")
            got = mm.cpu().numpy().reshape(C, S, 2)
            assert np.array_equal(got[..., 0], mn) and np.array_equal(got[..., 1], mx), (C, S)
            y = x * 1.05 + rng.normal(size=x.shape)                    # the resampled values overshoot the range here and there
            y.reshape(-1)[:4] = [mn[0, 0], mx[0, 0], np.nextafter(mn[0, 0], -np.inf), np.nextafter(mx[0, 0], np.inf)]
            yd = torch.from_numpy(y).to(dev)
            out = torch.full(x.shape, float("nan"), dtype=torch.float32, device=dev)
            check(lib().cf_slab_clip_to_f32(yd.data_ptr(), out.data_ptr(), C, A, S, B, mm.data_ptr(), _stream()), "cf_slab_clip_to_f32")
            same_bits(out.cpu().numpy(), slab_clip_f32(y, mn, mx))
            out.fill_(float("nan"))
            check(lib().cf_slab_clip_to_f32(yd.data_ptr(), out.data_ptr(), C, A, S, B, None, _stream()), "cf_slab_clip_to_f32")
            same_bits(out.cpu().numpy(), slab_clip_f32(y))             # minmax = NULL: plain rounding
    ratio_line("slab min / max / clip A=%d B=%d (C 1 / 2, S 1 / 5): differing values" % (A, B), 0.0, 0)
