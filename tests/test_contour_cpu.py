"""The host side of `python -m cineflow.score contour`, without a GPU: the parser, the pairing of flow files with contour files and the ED
image (every refusal raised from headers and shapes), the documents contour_tables / strain_tables build from hand-made rows, the C entry
points' argument checks (they run before any device call), and tests/_contour_refs.py -- the restatement the GPU tests hold the kernels
to -- against the reference's own stored output (tests/golden/strain.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _contour_refs as R
from _score_refs import case_names, make_patient, write_tree

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strain.npz")
NAN = float("nan")


def add_ed_image(root, patient, T, ed, shape, spacing=(1.25, 1.5, 10.0)):
    from cineflow.nifti import write_nifti
    path = os.path.join(root, "input", patient, case_names(patient, T)[ed] + "_0000.nii.gz")
    write_nifti(path, np.zeros(shape, np.float32), spacing=spacing)
    return path


# ------------------------------------------------------------------------------------------------ parser
def test_parser():
    from cineflow import score as S
    p = S.build_parser()
    a = p.parse_args(["contour", "-flow", "F", "-c", "C", "-i", "I"])
    assert vars(a) == {"command": "contour", "flow": "F", "c": "C", "i": "I", "layout": "predict", "mode": "from_ed"}
    for mode in ("from_ed", "from_ed_accumulation", "to_ed", "to_ed_accumulation"):
        a = p.parse_args(["contour", "-flow", "F", "-c", "C", "-i", "I", "--layout", "saver", "--mode", mode])
        assert (a.layout, a.mode) == ("saver", mode)
    for bad in (["contour", "-flow", "F", "-c", "C"], ["contour", "-flow", "F", "-i", "I"], ["contour", "-c", "C", "-i", "I"],
                ["contour", "-flow", "F", "-c", "C", "-i", "I", "--mode", "backwards"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    # the other sub-commands parse as before
    assert vars(p.parse_args(["seg", "-pred", "P", "-ref", "R"])) == {"command": "seg", "pred": "P", "ref": "R", "gt": "frame", "i": None, "layout": "predict"}
    assert vars(p.parse_args(["jacobian", "-flow", "F", "-l", "L"])) == {"command": "jacobian", "flow": "F", "l": "L", "i": None, "layout": "predict"}
    assert vars(p.parse_args(["ssim", "-flow", "F", "-i", "I"])) == {"command": "ssim", "flow": "F", "i": "I", "l": None, "layout": "predict", "win": 7}
    with pytest.raises(SystemExit):
        p.parse_args(["jacobian", "-flow", "F"])


# ------------------------------------------------------------------------------------------------ pairing
@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_pairing_and_arrays(tmp_path, layout):
    from cineflow import score as S
    T, ed, D, H, W = 12, 9, 2, 10, 8
    d = make_patient(3, T, D=D, H=H, W=W)
    out, gt, inp = write_tree(str(tmp_path), layout, "patientC", d, ed, 4)
    add_ed_image(str(tmp_path), "patientC", T, ed, (D, H, W))
    contours = R.make_contours(5, T, D, H, W)
    cfolder = R.write_contours(str(tmp_path), "patientC", contours)
    folder = S.patient_folders(out, layout, "Flow")["patientC"]
    cases, zoom = S.pair_contour_cases(folder, cfolder, inp, "patientC", ed)
    assert zoom == (1.25, 1.5)                                                   # pixdim[1], pixdim[2]: nibabel's get_zooms()[:2]
    flows, slices = cases[:T - 1], cases[T - 1:]
    assert [c.frame for c in flows] == [t + 1 for t in range(T) if t != ed]      # by frame number, two digits included; no ED flow
    assert all(c.path.endswith(c.name + ".npz") for c in flows)
    assert [c.name for c in slices] == ["patientC_slice01", "patientC_slice02"] and [c.frame for c in slices] == [0, 1]
    assert all(c.path.endswith(os.path.join("contour", "LV", c.name + ".npy")) and c.other.endswith(os.path.join("contour", "RV", c.name + ".npy"))
               for c in slices)
    loaded = [S._read_contour_case(c) for c in cases]
    assert loaded[0].dtype == np.float32 and loaded[0].shape == (H, W, D, 2)
    assert loaded[T - 1][0].shape == (T, 9, 4) and loaded[T - 1][1].shape == (T, 5, 2) and loaded[T][0].shape == (T, 11, 4)
    flow, pts, counts = S.contour_arrays(loaded[:T - 1], loaded[T - 1:], ed)
    assert flow.shape == (D, T, 2, W, H) and np.isnan(flow[:, 0]).all() and not np.isnan(flow[:, 1:]).any()
    assert counts.tolist() == [[9, 9, 5], [11, 11, 6]] and pts.shape == (D, T, 28, 2) and pts.dtype == np.float32
    order = list(range(ed, T)) + list(range(ed))
    lv, rv = contours[1]
    assert np.array_equal(pts[1, :, :11], (lv[:2].transpose(2, 1, 0)[order] - 1).astype(np.float32))              # endo, 0-based, ED first
    assert np.array_equal(pts[1, :, 11:22], (lv[2:].transpose(2, 1, 0)[order] - 1).astype(np.float32))            # epi
    assert np.array_equal(pts[1, :, 22:28], (rv.transpose(2, 1, 0)[order] - 1).astype(np.float32))
    assert not pts[0, :, 23:].any()                                                                                # padding
    assert np.array_equal(flow[1, 1, 0], d["flow"][order[1]][:, :, 1, 0].T)


def test_pairing_refusals(tmp_path):
    from cineflow import metrics, score as S, strain
    T, ed, D, H, W = 5, 1, 2, 10, 8
    d = make_patient(4, T, D=D, H=H, W=W)
    names = case_names("patientD", T)
    out, gt, inp = write_tree(str(tmp_path), "predict", "patientD", d, ed, 3)
    folder = S.patient_folders(out, "predict", "Flow")["patientD"]
    contours = R.make_contours(6, T, D, H, W)
    pair = lambda c: S.pair_contour_cases(folder, c, inp, "patientD", ed)          # noqa: E731
    # a missing slice file, LV or RV
    c1 = R.write_contours(str(tmp_path / "a"), "patientD", contours, skip={("LV", 1)})
    with pytest.raises(ValueError, match="no contour file .*LV.patientD_slice02.npy"):
        pair(c1)
    c2 = R.write_contours(str(tmp_path / "b"), "patientD", contours, skip={("RV", 0)})
    with pytest.raises(ValueError, match="no contour file .*RV.patientD_slice01.npy"):
        pair(c2)
    # a frame count different from the number of flow files + 1
    c3 = R.write_contours(str(tmp_path / "c"), "patientD", R.make_contours(6, T + 1, D, H, W))
    with pytest.raises(ValueError, match="patientD_slice01.npy: 6 frames, but 4 flow files"):
        pair(c3)
    # an LV file that is not [4, P, T]: endo and epi points cannot pair up
    c4 = R.write_contours(str(tmp_path / "d"), "patientD", [(lv[:3], rv) for lv, rv in contours])
    with pytest.raises(ValueError, match=r"LV.patientD_slice01.npy: shape \(3, 9, 5\), expected \[4, P, T\]"):
        pair(c4)
    # no ED image: no pixel spacing
    good = R.write_contours(str(tmp_path / "e"), "patientD", contours)
    with pytest.raises(ValueError, match=names[ed] + ": no image"):
        pair(good)
    add_ed_image(str(tmp_path), "patientD", T, ed, (D, H, W))
    assert len(pair(good)[0]) == T - 1 + D
    # the refusals reach the sub-command before any device work (no GPU here)
    with pytest.raises(ValueError, match="6 frames, but 4 flow files"):
        S.main(["contour", "-flow", out, "-c", c3, "-i", inp])
    # a flow file missing in the middle of the cine
    os.remove(os.path.join(folder, names[3] + ".npz"))
    with pytest.raises(ValueError, match="patientD: flow files of frames \\[1, 3, 5\\]"):
        pair(good)
    # unequal endo / epi counts: refused from the counts alone, before any device work, by the patient-level call and by the wrappers
    flow = np.zeros((1, 3, 2, 4, 4), np.float32)
    pts = np.zeros((1, 3, 8, 2), np.float32)
    with pytest.raises(ValueError, match="slice 0: 3 endo and 4 epi points"):
        strain.track_patient(flow, pts, np.array([[3, 4, 1]]), "from_ed", zoom=(1.0, 1.0))
    with pytest.raises(ValueError, match="slice 0: 3 endo and 4 epi points"):
        metrics.contour_strain_table(np.zeros((1, 2, 8, 2), np.float32), pts[:, 0], np.array([[3, 4, 1]]), (1.0, 1.0))
    with pytest.raises(ValueError, match="more points than the padded row of 8"):
        metrics.contour_track_table(flow, pts, np.array([[3, 4, 2]]), "from_ed")
    with pytest.raises(ValueError, match="takes no zoom"):
        strain.track_patient(flow, pts, np.array([[3, 3, 1]]), "to_ed", zoom=(1.0, 1.0))
    with pytest.raises(ValueError, match="mode must be one of"):
        strain.track_patient(flow, pts, np.array([[3, 3, 1]]), "backwards")


# ------------------------------------------------------------------------------------------------ documents
def test_rows_and_tables():
    from cineflow import score as S
    assert S.CONTOUR_COLUMNS == ["Name", "slice_number", "ENDO", "EPI", "RV", "Average"]
    ea = np.arange(2 * 3 * 3, dtype=np.float64).reshape(2, 3, 3) / 8                       # patient a: D=2, T-1=3
    eb = np.full((1, 2, 3), 2.0)
    eb[0, :, 2] = NAN                                                                      # patient b: one slice without RV points
    per = {"a": S.contour_rows("a", ea), "b": S.contour_rows("b", eb)}
    assert [list(e) for e in per["a"]] == [["Name", "slice_number", "ENDO", "EPI", "RV"]] * 2
    assert per["a"][1] == {"Name": "a", "slice_number": 1, "ENDO": ea[1, :, 0].tolist(), "EPI": ea[1, :, 1].tolist(), "RV": ea[1, :, 2].tolist()}
    doc, rows = S.contour_tables({"a": per["a"]})
    assert set(doc) == {"all", "mean", "std"} and doc["all"] == {"a": [dict(e) for e in per["a"]]}
    assert [list(r) for r in rows] == [S.CONTOUR_COLUMNS] * 2
    for r, e in zip(rows, ea):
        assert [r["ENDO"], r["EPI"], r["RV"]] == e.mean(0).tolist() and r["Average"] == (r["ENDO"] + r["EPI"] + r["RV"]) / 3
    for i, k in enumerate(S.CONTOUR_STRUCTURES):
        per_slice = np.array([ea[0, :, i].mean(), ea[1, :, i].mean()])
        assert doc["mean"][k] == per_slice.mean() and doc["std"][k] == per_slice.std()
    # the restatement builds the same documents
    rdoc, rrows, sdoc = R.documents({"a": (ea, None, 0)})
    assert rdoc == doc and [dict(r) for r in rows] == rrows and sdoc is None
    # a slice without RV points: NaN in its row, its Average and the document's RV mean and std, nowhere else
    doc, rows = S.contour_tables(per)
    assert list(doc["all"]) == ["a", "b"] and len(rows) == 3
    assert np.isnan(rows[2]["RV"]) and np.isnan(rows[2]["Average"]) and rows[2]["ENDO"] == 2.0 and not np.isnan(rows[1]["Average"])
    assert np.isnan(doc["mean"]["RV"]) and np.isnan(doc["std"]["RV"]) and not np.isnan(doc["mean"]["ENDO"])

    # strain documents: curves rolled back to the acquisition order, smoothness per slice, the mean over patients of per-patient means
    T = 6
    t = np.arange(T, dtype=np.float64)
    curves = np.stack([np.stack([-0.1 * np.sin(np.pi * t / T) * (d + 1), -0.05 * t * (T - t) / 9], axis=-1) for d in range(2)])
    entries = S.strain_rows("a", curves, to_roll=4)
    assert [list(e) for e in entries] == [["Name", "slice_number", "radial_strain", "circ_strain", "smooth"]] * 2
    for d, e in enumerate(entries):
        assert e["radial_strain"] == np.roll(curves[d, :, 0], -4).tolist() and e["circ_strain"] == np.roll(curves[d, :, 1], -4).tolist()
        assert e["radial_strain"][2] == 0.0                                                # the ED frame (row 0) sits at index T - to_roll
        want = (R.smoothness(e["radial_strain"]) + R.smoothness(e["circ_strain"])) / 2
        assert e["smooth"] == pytest.approx(want, rel=1e-12) and want > 0
    other = S.strain_rows("b", curves[:1] * 2, to_roll=1)
    sdoc = S.strain_tables({"a": entries, "b": other})
    assert set(sdoc) == {"all", "mean"} and list(sdoc["all"]) == ["a", "b"]
    assert sdoc["mean"] == pytest.approx(np.mean([np.mean([e["smooth"] for e in entries]), other[0]["smooth"]]), rel=1e-12)
    _, _, rs = R.documents({"a": (ea, curves, 4)})
    assert rs["all"]["a"][1]["radial_strain"] == entries[1]["radial_strain"] and rs["mean"] == pytest.approx(np.mean([e["smooth"] for e in entries]), rel=1e-12)


# ------------------------------------------------------------------------------------------------ the entry points' argument checks
def test_entry_points_are_declared_and_refuse_bad_arguments():
    from cineflow import _lib
    assert len(_lib.SIGNATURES["cf_contour_track_table"]) == 13 and len(_lib.SIGNATURES["cf_contour_strain_table"]) == 12
    h = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    bad = -1                                                      # CF_ERR_ARG: returned before any device call

    def counts(*rows):
        return np.ascontiguousarray(np.array(rows, dtype=np.int32))

    def track(flow=p, pts=p, c=counts((2, 2, 1)), cd=p, D=1, T=3, A=4, B=5, Pmax=8, mode=0, pos=p, table=p):
        rc = h.cf_contour_track_table(flow, pts, None if c is None else c.ctypes.data, cd, D, T, A, B, Pmax, mode, pos, table, None)
        return rc, h.cf_last_error().decode()

    def strain(pos=p, ed=p, stride=16, c=counts((2, 2, 1)), cd=p, D=1, T=3, Pmax=8, table=p):
        rc = h.cf_contour_strain_table(pos, ed, stride, None if c is None else c.ctypes.data, cd, D, T, Pmax, 1.25, 1.25, table, None)
        return rc, h.cf_last_error().decode()
    for kw in (dict(flow=None), dict(pts=None), dict(c=None), dict(cd=None), dict(pos=None), dict(table=None)):
        rc, msg = track(**kw)
        assert rc == bad and "cf_contour_track_table: null pointer" in msg, (kw, rc, msg)
    for kw, text in ((dict(T=1), "bad shape"), (dict(A=1), "bad shape"), (dict(B=1), "bad shape"), (dict(D=0), "bad shape"), (dict(Pmax=0), "bad shape"),
                     (dict(D=65536), "too large"), (dict(mode=4), "mode must be 0"), (dict(mode=-1), "mode must be 0"),
                     (dict(c=counts((2, -1, 1))), "slice 0: negative count"), (dict(c=counts((4, 4, 1))), "exceed the padded row Pmax=8"),
                     (dict(D=2, c=counts((2, 2, 1), (3, 3, 3))), "slice 1: 3 + 3 + 3 points exceed")):
        rc, msg = track(**kw)
        assert rc == bad and text in msg, (kw, rc, msg)
    for kw in (dict(pos=None), dict(ed=None), dict(c=None), dict(cd=None), dict(table=None)):
        rc, msg = strain(**kw)
        assert rc == bad and "cf_contour_strain_table: null pointer" in msg, (kw, rc, msg)
    for kw, text in ((dict(T=1), "bad shape"), (dict(D=0), "bad shape"), (dict(Pmax=0), "bad shape"), (dict(stride=14), "ed_stride=14"),
                     (dict(stride=17), "ed_stride=17"), (dict(c=counts((2, 3, 1))), "slice 0: 2 endo and 3 epi points"),
                     (dict(D=2, c=counts((2, 2, 1), (1, 0, 0))), "slice 1: 1 endo and 0 epi points"), (dict(c=counts((5, 5, 0))), "exceed the padded row")):
        rc, msg = strain(**kw)
        assert rc == bad and text in msg, (kw, rc, msg)


# ------------------------------------------------------------------------------------------------ the restatement against the golden ring
def _ring():
    g = np.load(GOLD)
    counts = (int(g["ring_split"][0]), int(g["ring_split"][1] - g["ring_split"][0]), int(g["ring_con_all"].shape[1] - g["ring_split"][1]))
    return g, counts


@pytest.mark.parametrize("mode", ["from_ed_accumulation", "to_ed_accumulation", "to_ed"])
def test_refs_reproduce_the_stored_tracking_errors(mode):
    g, counts = _ring()
    pos = R.positions(g["ring_flow"], g["ring_con_all"], mode)
    e = R.error_table(g["ring_con_all"], pos, counts, mode)
    assert e.shape == g["ring_err_" + mode].shape == (6, 3) and e.dtype == np.float64
    assert float(np.abs(e - g["ring_err_" + mode]).max()) <= 1e-4             # the bar of tests/test_strain.py
    assert not np.isnan(pos).any()                                            # frame 0 of the flow is NaN and is never read


def test_refs_reproduce_the_stored_strain_curves():
    g, _ = _ring()
    con = np.concatenate([g["ring_contours"][0], g["ring_contours"][1]], axis=1)                  # T, 2 n, 2
    n = g["ring_contours"].shape[2]
    pos = R.positions(g["ring_flow"], con, "from_ed")
    tab = R.strain_table(pos, con[0], n, (1.25, 1.25))
    assert tab.shape == (7, 2) and (tab[0] == 0).all()
    assert float(np.abs(np.roll(tab[:, 0], -2) - g["ring_radial"]).max()) <= 1e-5                 # to_roll = 2 in the stored run; test_strain.py's bar
    assert float(np.abs(np.roll(tab[:, 1], -2) - g["ring_circ"]).max()) <= 1e-5
    smooth = (R.smoothness(np.roll(tab[:, 0], -2)) + R.smoothness(np.roll(tab[:, 1], -2))) / 2
    assert abs(smooth - float(g["ring_smooth"])) <= 1e-4 * max(1.0, abs(float(g["ring_smooth"])))


def test_from_ed_on_the_ring_is_track_from_ed_minus_ground_truth():
    from oracle import strain as OS
    g, counts = _ring()
    con = g["ring_con_all"]
    pos = R.positions(g["ring_flow"], con, "from_ed")
    first = torch.from_numpy(con[0].T.copy())[None]                                               # 1, 2, P: all points as one structure
    tracked = OS.track_from_ed(first, torch.from_numpy(g["ring_flow"]).float())[1:, 0].permute(0, 2, 1).numpy()
    assert np.array_equal(pos, tracked)
    want = np.linalg.norm(tracked.astype(np.float64) - con[1:].astype(np.float64), axis=2)
    assert np.array_equal(R.point_errors(con, pos, "from_ed"), want)
    tab = R.error_table(con, pos, counts, "from_ed")
    assert np.allclose(tab[:, 0], want[:, :24].mean(1), rtol=0, atol=1e-12) and np.allclose(tab[:, 2], want[:, 48:].mean(1), rtol=0, atol=1e-12)
    assert 0 < tab.max() < 5 and not np.isnan(tab).any()
    # a structure without points is NaN, the others are unchanged
    t2 = R.error_table(con[:, :48], pos[:, :48], (24, 24, 0), "from_ed")
    assert np.isnan(t2[:, 2]).all() and np.array_equal(t2[:, :2], tab[:, :2])
