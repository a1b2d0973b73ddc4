"""cf_contour_track_table / cf_contour_strain_table (csrc/contour.hip) through cineflow.metrics.contour_track_table /
contour_strain_table and cineflow.strain.track_patient.

  * pos: bit-identical to the same chains walked one ops.sample_points call per step on the same device (tests/_contour_refs.positions
    with the device as its sampler; the chain's adds are single IEEE fp32 adds on either side), in all four modes; padding points are 0.
  * table: against the fp64 restatement evaluated on the device's own pos, 1e-10 -- only the order of summation differs (a few hundred
    fp64 terms of order 1 to 100: 1e-13 at most).  NaN meets NaN (a structure without points).
  * strain: against the fp64 restatement on the device's own pos, 1e-10 relative to max(1, |value|), NaN meets NaN (a one-point contour
    is 0 / 0 in the circumferential direction).
  * the reference's stored ring (tests/golden/strain.npz): errors within 1e-4, strain curves within 1e-5, the bars of tests/test_strain.py.
  * no NaN leaks from frame 0 of the flow, which is NaN in every case here; two runs are bit-identical.

Shapes: the smallest legal map 2 x 3, 7 x 5 and 33 x 65; T = 2 (one flow), 3 and 30; D = 1 and 3 with different counts per slice (padding);
counts (1, 1, 0), (63, 63, 2), (64, 64, 65) and (257, 257, 130) around the wave and workgroup sizes; in every slice points exactly on the
last row and column and points outside the map; a T = 30 case whose flow carries the points out of a 7 x 5 map in mid-chain."""
import numpy as np
import pytest
import torch

import _contour_refs as R
from _kernel_refs import ratio_line

pytestmark = pytest.mark.gpu

TABLE_BAR = 1e-10
# name: (A, B, T, counts per slice, flow amplitude in pixels)
CASES = {
    "2x3 T2 (1,1,0)": (2, 3, 2, [(1, 1, 0)], 0.4),
    "7x5 T3 D3 (63,63,2)": (7, 5, 3, [(63, 63, 2), (5, 5, 7), (1, 1, 0)], 0.8),
    "33x65 T3 (64,64,65)": (33, 65, 3, [(64, 64, 65)], 2.0),
    "33x65 T2 D3 (257,257,130)": (33, 65, 2, [(257, 257, 130), (64, 64, 65), (3, 3, 1)], 2.0),
    "7x5 T30 leaving the map": (7, 5, 30, [(6, 6, 3)], 1.5),
}


def make_case(seed, A, B, T, counts, amplitude):
    """flow [D, T, 2, A, B] with frame 0 NaN, pts [D, T, Pmax, 2] (x along B, y along A) padded with a value that must never be read
    into a result, counts [D, 3].  Point 0 of a slice sits on the last row and column; with four points or more, point 1 lies outside
    the map, point 2 on the last column and point 3 on the last row."""
    rng = np.random.default_rng(seed)
    D, Pmax = len(counts), max(sum(c) for c in counts)
    flow = rng.normal(0.0, amplitude, size=(D, T, 2, A, B)).astype(np.float32)
    flow[:, 0] = np.nan
    pts = np.full((D, T, Pmax, 2), 1.0e6, np.float32)
    for d, c in enumerate(counts):
        n = sum(c)
        p = rng.uniform(0.0, 1.0, size=(T, n, 2)) * np.array([B - 1, A - 1]) + rng.normal(0, 0.3, size=(T, n, 2))
        p[:, 0] = (B - 1, A - 1)
        if n >= 4:
            p[:, 1] = (-1.25, A + 0.5)
            p[:, 2, 0] = B - 1
            p[:, 3, 1] = A - 1
        pts[d, :, :n] = p.astype(np.float32)
    return flow, pts, np.array(counts, dtype=np.int32)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def results(dev):
    """(case, mode) -> dict(pos, table: the kernel's, as numpy; chain: the per-launch positions per slice; again: a second run's bits equal)"""
    from cineflow import metrics
    sampler = R.device_sampler(dev)
    out = {}
    for i, (name, (A, B, T, counts, amp)) in enumerate(CASES.items()):
        flow, pts, cnt = make_case(100 + i, A, B, T, counts, amp)
        for mode in R.MODES:
            pos, table = metrics.contour_track_table(flow, pts, cnt, mode)
            pos2, table2 = metrics.contour_track_table(torch.from_numpy(flow).to(dev), torch.from_numpy(pts).to(dev), cnt, R.MODES.index(mode))
            again = np.array_equal(bits(pos), bits(pos2)) and np.array_equal(bits(table), bits(table2))
            chain = [R.positions(flow[d], pts[d, :, :sum(c)], mode, sampler) for d, c in enumerate(counts)]
            out[name, mode] = dict(flow=flow, pts=pts, counts=cnt, pos=pos.cpu().numpy(), pos_dev=pos, table=table.cpu().numpy(), chain=chain, again=again)
    return out


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_positions_are_the_bits_of_chained_sample_points_calls(results, case, mode):
    r = results[case, mode]
    D, T = r["pts"].shape[:2]
    assert r["pos"].shape == (D, T - 1, r["pts"].shape[2], 2) and r["pos"].dtype == np.float32
    for d in range(D):
        n = int(r["counts"][d].sum())
        assert not np.isnan(r["chain"][d]).any(), "the restated chain read the NaN frame"
        assert np.array_equal(r["pos"][d, :, :n], r["chain"][d]), (case, mode, d)
        assert not r["pos"][d, :, n:].any(), "padding points are written as 0"
    assert r["again"], "two runs must give the same bits"


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_table_matches_the_fp64_restatement_on_the_device_positions(results, case, mode):
    r = results[case, mode]
    D, T = r["pts"].shape[:2]
    assert r["table"].shape == (D, T - 1, 3) and r["table"].dtype == np.float64
    worst = 0.0
    for d in range(D):
        c = r["counts"][d]
        want = R.error_table(r["pts"][d], r["pos"][d], c, mode)
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(r["table"][d])), (case, mode, d)
        assert np.array_equal(nan.all(0), c == 0) and np.array_equal(nan.any(0), c == 0), "NaN exactly for the structures without points"
        if (~nan).any():
            worst = max(worst, float(np.abs(r["table"][d] - want)[~nan].max()))
    print()
    assert ratio_line("contour table %s %s" % (case, mode), worst, TABLE_BAR) <= 1


def test_leaving_the_map_in_mid_chain_is_exercised(results):
    """the T = 30 case: points start inside, and the chain carries most of them outside, where the flow reads as zero and they stop"""
    r = results["7x5 T30 leaving the map", "from_ed_accumulation"]
    pos = r["pos"][0][:, 4:15]                                                     # the points that start inside the map
    start = r["pts"][0, 0, 4:15]
    inside = lambda p: (p[..., 0] >= 0) & (p[..., 0] <= 4) & (p[..., 1] >= 0) & (p[..., 1] <= 6)          # noqa: E731
    assert inside(start).sum() >= 8
    gone = ~inside(pos[-1]) & inside(start)
    assert gone.sum() >= 3, "the flow is too weak to carry points out of the map"
    far = (pos[-2][..., 0] < -1) | (pos[-2][..., 0] > 5) | (pos[-2][..., 1] < -1) | (pos[-2][..., 1] > 7)
    assert far.sum() >= 3 and np.array_equal(pos[-1][far], pos[-2][far]), "a point a pixel or more outside samples zeros and stays"


@pytest.mark.parametrize("case", list(CASES))
def test_strain_table_matches_the_fp64_restatement(dev, results, case):
    from cineflow import metrics
    r = results[case, "from_ed"]
    zoom = (1.25, 1.5)
    D, T = r["pts"].shape[:2]
    ed = torch.from_numpy(r["pts"]).to(dev)[:, 0]                                  # a strided view of the [D, T, Pmax, 2] array, read in place
    tab = metrics.contour_strain_table(r["pos_dev"], ed, r["counts"], zoom)
    tab2 = metrics.contour_strain_table(r["pos"], r["pts"][:, 0].copy(), r["counts"], zoom)
    assert np.array_equal(bits(tab), bits(tab2)), "two runs, strided and contiguous ED points: the same bits"
    tab = tab.cpu().numpy()
    assert tab.shape == (D, T, 2) and tab.dtype == np.float64
    worst = 0.0
    for d in range(D):
        n = int(r["counts"][d][0])
        want = R.strain_table(r["pos"][d], r["pts"][d, 0], n, zoom)
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(tab[d])), (case, d)
        if n == 1:
            assert nan[:, 1].all() and not nan[:, 0].any(), "one point per contour: circumferential strain is 0 / 0, radial is not"
        assert (tab[d, 0][~nan[0]] == 0).all(), "row 0 is the ED frame against itself"
        if (~nan).any():
            worst = max(worst, float((np.abs(tab[d] - want) / np.maximum(1.0, np.abs(want)))[~nan].max()))
    print()
    assert ratio_line("contour strain %s" % case, worst, TABLE_BAR) <= 1


def test_refusals_come_before_the_device(dev):
    from cineflow import metrics
    flow, pts, cnt = make_case(1, 7, 5, 3, [(3, 4, 1)], 0.5)
    pos, _ = metrics.contour_track_table(flow, pts, cnt, "from_ed")
    with pytest.raises(ValueError, match="3 endo and 4 epi points"):
        metrics.contour_strain_table(pos, pts[:, 0], cnt, (1.0, 1.0))
    with pytest.raises(ValueError, match="flow has to be"):
        metrics.contour_track_table(flow[:, :2], pts, cnt, "from_ed")


# ------------------------------------------------------------------------------------------------ the reference's stored ring
@pytest.fixture(scope="module")
def ring():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strain.npz"))
    s = g["ring_split"]
    return g, np.array([[int(s[0]), int(s[1] - s[0]), int(g["ring_con_all"].shape[1] - s[1])]], dtype=np.int32)


@pytest.mark.parametrize("mode", ["from_ed_accumulation", "to_ed_accumulation", "to_ed"])
def test_ring_tracking_errors(dev, ring, mode):
    from cineflow import strain as S
    g, counts = ring
    assert np.isnan(g["ring_flow"][0]).all()
    res = S.track_patient(g["ring_flow"][None], g["ring_con_all"][None], counts, mode)
    assert set(res) == {"errors"} and res["errors"].shape == (1, 6, 3) and not np.isnan(res["errors"]).any()
    print()
    assert ratio_line("ring " + mode, float(np.abs(res["errors"][0] - g["ring_err_" + mode]).max()), 1e-4) <= 1


def test_ring_from_ed_and_strain(dev, ring):
    from cineflow import metrics, strain as S
    g, _ = ring
    con = np.concatenate([g["ring_contours"][0], g["ring_contours"][1]], axis=1)[None]             # 1, T, 2 n, 2
    n = g["ring_contours"].shape[2]
    counts = np.array([[n, n, 0]], dtype=np.int32)
    res = S.track_patient(g["ring_flow"][None], con, counts, "from_ed", zoom=(1.25, 1.25))
    assert set(res) == {"errors", "strain"} and res["strain"].shape == (1, 7, 2)
    assert np.isnan(res["errors"][0, :, 2]).all() and not np.isnan(res["errors"][0, :, :2]).any() and not np.isnan(res["strain"]).any()
    print()
    assert ratio_line("ring radial", float(np.abs(np.roll(res["strain"][0, :, 0], -2) - g["ring_radial"]).max()), 1e-5) <= 1
    assert ratio_line("ring circ", float(np.abs(np.roll(res["strain"][0, :, 1], -2) - g["ring_circ"]).max()), 1e-5) <= 1
    # the patient-level call returns the two tables of the wrappers, bit for bit
    pos, table = metrics.contour_track_table(g["ring_flow"][None], con, counts, "from_ed")
    curves = metrics.contour_strain_table(pos, con[:, 0], counts, (1.25, 1.25))
    assert np.array_equal(bits(table), bits(torch.from_numpy(res["errors"]))) and np.array_equal(bits(curves), bits(torch.from_numpy(res["strain"])))
    # mode from_ed: the tracked positions of strain.track_from_ed minus the ground truth, and the per-launch function's new mode
    first = torch.from_numpy(con[0, 0].T.copy())[None]
    tracked = S.track_from_ed(first, torch.from_numpy(g["ring_flow"]).float())[1:, 0].permute(0, 2, 1).numpy()
    assert np.array_equal(pos.cpu().numpy()[0], tracked)
    want = np.linalg.norm(tracked.astype(np.float64) - con[0, 1:].astype(np.float64), axis=2)
    assert float(np.abs(res["errors"][0, :, 0] - want[:, :n].mean(1)).max()) <= TABLE_BAR
    # fp32 differences of coordinates up to 56 (half an ulp is 1.9e-6 per component) in the per-launch function: 1e-5
    per_launch = S.contour_tracking_error(g["ring_flow"], g["ring_con_all"], g["ring_split"], "from_ed")
    full = S.track_patient(g["ring_flow"][None], g["ring_con_all"][None], ring[1], "from_ed")["errors"][0]
    assert per_launch.shape == (6, 3) and float(np.abs(per_launch - full).max()) <= 1e-5
