"""The host side of `python -m cineflow.score ssim`, without a GPU: the parser, the pairing of flow files with images and the ED label
volume (every refusal raised from headers), the documents ssim_rows / ssim_tables build from hand-made rows, and the C entry point's
argument checks, which run before any device call."""
import ctypes
import os

import numpy as np
import pytest

from _score_refs import case_names, make_patient, write_tree

NAN = float("nan")


def add_images(root, patient, T, shape, seed=0, skip=()):
    """<root>/input/<patient>/<case>_0000.nii.gz, float32 [Z, Y, X] = shape"""
    from cineflow.nifti import write_nifti
    rng = np.random.default_rng(seed)
    for t, name in enumerate(case_names(patient, T)):
        if t not in skip:
            write_nifti(os.path.join(root, "input", patient, name + "_0000.nii.gz"), rng.normal(300, 40, size=shape).astype(np.float32))


# ------------------------------------------------------------------------------------------------ parser
def test_parser():
    from cineflow import score as S
    p = S.build_parser()
    a = p.parse_args(["ssim", "-flow", "F", "-i", "I"])
    assert vars(a) == {"command": "ssim", "flow": "F", "i": "I", "l": None, "layout": "predict", "win": 7}
    a = p.parse_args(["ssim", "-flow", "F", "-i", "I", "-l", "L", "--layout", "saver", "--win", "11"])
    assert (a.l, a.layout, a.win) == ("L", "saver", 11)
    with pytest.raises(SystemExit):
        p.parse_args(["ssim", "-flow", "F"])
    with pytest.raises(SystemExit):
        p.parse_args(["ssim", "-i", "I"])
    # the other sub-commands parse as before
    assert vars(p.parse_args(["seg", "-pred", "P", "-ref", "R"])) == {"command": "seg", "pred": "P", "ref": "R", "gt": "frame", "i": None, "layout": "predict"}
    assert vars(p.parse_args(["jacobian", "-flow", "F", "-l", "L"])) == {"command": "jacobian", "flow": "F", "l": "L", "i": None, "layout": "predict"}
    with pytest.raises(SystemExit):
        p.parse_args(["jacobian", "-flow", "F"])


# ------------------------------------------------------------------------------------------------ pairing
@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_pairing(tmp_path, layout):
    from cineflow import score as S
    T, ed = 12, 9
    d = make_patient(3, T, D=2, H=10, W=8)
    out, gt, inp = write_tree(str(tmp_path), layout, "patientC", d, ed, 4)
    add_images(str(tmp_path), "patientC", T, (2, 10, 8))
    folder = S.patient_folders(out, layout, "Flow")["patientC"]
    labels = out if layout == "predict" else os.path.join(out, "Postprocessed", "Segmentation")
    cases = S.pair_ssim_cases(folder, inp, "patientC", ed, labels)
    names = case_names("patientC", T)
    assert cases[0].name == names[ed] and cases[0].frame == ed + 1 and cases[0].path.endswith(names[ed] + "_0000.nii.gz")
    assert os.path.basename(cases[0].other) == names[ed] + ".nii.gz"
    assert [c.frame for c in cases[1:]] == [t + 1 for t in range(T) if t != ed]            # by frame number, two digits included; no ED flow
    assert all(c.path.endswith(c.name + ".npz") and c.other.endswith(c.name + "_0000.nii.gz") for c in cases[1:])
    assert S.pair_ssim_cases(folder, inp, "patientC", ed)[0].other is None
    fixed, lab = S._read_ssim_case(cases[0])
    flow, img = S._read_ssim_case(cases[1])
    assert fixed.dtype == np.float64 and fixed.shape == (10, 8, 2) and lab.dtype == np.uint8 and lab.shape == (10, 8, 2)
    assert np.array_equal(lab, d["gt"][ed].transpose(1, 2, 0))
    assert flow.dtype == np.float32 and flow.shape == (10, 8, 2, 2) and img.dtype == np.float32 and img.shape == (10, 8, 2)


def test_pairing_refusals(tmp_path):
    from cineflow import score as S
    T, ed = 4, 1
    d = make_patient(4, T, D=2, H=10, W=8)
    names = case_names("patientD", T)
    out, gt, inp = write_tree(str(tmp_path), "predict", "patientD", d, ed, 3)
    folder = S.patient_folders(out, "predict", "Flow")["patientD"]
    add_images(str(tmp_path), "patientD", T, (2, 10, 8), skip=(2,))
    with pytest.raises(ValueError, match=names[2] + ": no image"):
        S.pair_ssim_cases(folder, inp, "patientD", ed)
    add_images(str(tmp_path), "patientD", T, (2, 10, 8), skip=(ed,))
    os.remove(os.path.join(inp, "patientD", names[ed] + "_0000.nii.gz"))
    with pytest.raises(ValueError, match=names[ed] + ": no image"):
        S.pair_ssim_cases(folder, inp, "patientD", ed)
    add_images(str(tmp_path), "patientD", T, (2, 10, 8))
    assert len(S.pair_ssim_cases(folder, inp, "patientD", ed, out)) == T
    empty = str(tmp_path / "nolabels")
    os.makedirs(empty)
    with pytest.raises(ValueError, match=names[ed] + ": no label volume"):
        S.pair_ssim_cases(folder, inp, "patientD", ed, empty)
    from cineflow.nifti import write_nifti
    write_nifti(os.path.join(inp, "patientD", names[3] + "_0000.nii.gz"), np.zeros((2, 8, 10), np.float32))
    with pytest.raises(ValueError, match=names[3] + ": image .* the flow \\[H, W, D\\] = \\(10, 8, 2\\)"):
        S.pair_ssim_cases(folder, inp, "patientD", ed)
    add_images(str(tmp_path), "patientD", T, (2, 10, 8))
    write_nifti(os.path.join(inp, "patientD", names[ed] + "_0000.nii.gz"), np.zeros((3, 10, 8), np.float32))
    with pytest.raises(ValueError, match=names[ed] + ": image"):
        S.pair_ssim_cases(folder, inp, "patientD", ed)
    # the refusals reach the sub-command before any device work (no GPU here)
    with pytest.raises(ValueError, match=names[ed] + ": image"):
        S.main(["ssim", "-flow", out, "-i", inp])


# ------------------------------------------------------------------------------------------------ documents
def _stats(T, D, structures=True, nan_at=()):
    """hand-made cine_ssim_table rows: SSIM_whole = d + t / 100, the structures 0.1, 0.2, 0.3 below it"""
    rows = []
    for d in range(D):
        for t in range(T):
            w = d + t / 100
            r = {"SSIM_whole": w}
            if structures:
                r.update({"SSIM_rv": w - 0.1, "SSIM_myo": NAN if (d, t) in nan_at else w - 0.2, "SSIM_lv": w - 0.3})
                r["SSIM_mean"] = (r["SSIM_rv"] + r["SSIM_myo"] + r["SSIM_lv"]) / 3
            rows.append(r)
    return rows


def test_rows_and_tables():
    from cineflow import score as S
    assert S.SSIM_COLUMNS == ["Name", "slice_number", "SSIM"]
    assert S.SSIM_ALL_COLUMNS == ["Name", "slice_number", "SSIM_mean", "SSIM_rv", "SSIM_myo", "SSIM_lv", "SSIM_whole",
                                  "ES_SSIM_mean", "ES_SSIM_rv", "ES_SSIM_myo", "ES_SSIM_lv", "ES_SSIM_whole"]
    frames = [1, 2, 4, 5, 11]                                     # ED = frame 3; positions 0..4
    stats = _stats(5, 2, nan_at={(1, 3)})
    entries, entries_all = S.ssim_rows("p", frames, stats, 3, 5)
    assert len(entries) == len(entries_all) == 2
    order = [2, 3, 4, 0, 1]                                       # frames 4, 5, 11, then 1, 2
    for d in (0, 1):
        assert list(entries[d]) == S.SSIM_COLUMNS and list(entries_all[d]) == S.SSIM_ALL_COLUMNS
        assert (entries[d]["Name"], entries[d]["slice_number"]) == ("p", d) == (entries_all[d]["Name"], entries_all[d]["slice_number"])
        assert entries[d]["SSIM"] == [d + t / 100 for t in order] == entries_all[d]["SSIM_whole"]
        assert entries_all[d]["SSIM_rv"] == [d + t / 100 - 0.1 for t in order]
        assert entries_all[d]["ES_SSIM_whole"] == d + 3 / 100 and entries_all[d]["ES_SSIM_lv"] == d + 3 / 100 - 0.3          # frame 5 = position 3
    assert np.isnan(entries_all[1]["SSIM_myo"][1]) and np.isnan(entries_all[1]["SSIM_mean"][1]) and np.isnan(entries_all[1]["ES_SSIM_myo"])
    assert not np.isnan(entries_all[1]["SSIM_rv"]).any() and not np.isnan(entries_all[0]["ES_SSIM_mean"])
    # the ES frame has no flow file (it is the ED frame, or absent): NaN in every ES column
    for es in (3, 7):
        _, ea = S.ssim_rows("p", frames, stats, 3, es)
        assert all(np.isnan(ea[d]["ES_" + k]) for d in (0, 1) for k in S.SSIM_KEYS)
    # without structures there are no `all` entries
    e, ea = S.ssim_rows("p", frames, _stats(5, 2, structures=False), 3, 5)
    assert ea == [] and e == entries

    doc, rows = S.ssim_tables(entries, "SSIM")
    assert set(doc) == {"all", "mean"} and doc["all"] == [dict(x) for x in entries]
    assert [list(r) for r in rows] == [S.SSIM_COLUMNS] * 2
    assert [r["SSIM"] for r in rows] == [float(np.mean(x["SSIM"])) for x in entries]
    assert doc["mean"] == float(np.mean([r["SSIM"] for r in rows]))
    doc_all, rows_all = S.ssim_tables(entries_all, "SSIM_mean")
    assert [list(r) for r in rows_all] == [S.SSIM_ALL_COLUMNS] * 2
    for r, x in zip(rows_all, entries_all):
        for k in S.SSIM_KEYS:
            want = float(np.mean(x[k]))
            assert (np.isnan(r[k]) and np.isnan(want)) or r[k] == want
            assert (np.isnan(r["ES_" + k]) and np.isnan(x["ES_" + k])) or r["ES_" + k] == x["ES_" + k]
    assert not np.isnan(rows_all[0]["SSIM_mean"]) and np.isnan(rows_all[1]["SSIM_mean"]) and np.isnan(rows_all[1]["SSIM_myo"])
    assert not np.isnan(rows_all[1]["SSIM_rv"])
    assert np.isnan(doc_all["mean"])                              # plain means: one NaN slice makes the document's mean NaN
    assert S.ssim_tables(entries_all[:1], "SSIM_mean")[0]["mean"] == rows_all[0]["SSIM_mean"]


# ------------------------------------------------------------------------------------------------ the entry point's argument checks
def test_entry_point_is_declared_and_refuses_bad_arguments():
    from cineflow import _lib
    assert len(_lib.SIGNATURES["cf_cine_ssim_table"]) == 16
    h = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)

    def call(fixed=p, reg=p, lab=None, T=1, D=1, H=20, W=20, K=0, win=7, rng=p, part=p, table=p):
        rc = h.cf_cine_ssim_table(fixed, reg, lab, T, D, H, W, K, win, 0.01, 0.03, 49 / 48.0, rng, part, table, None)
        return rc, h.cf_last_error().decode()
    bad = -1                                                      # CF_ERR_ARG: returned before any device call
    for kw in (dict(fixed=None), dict(reg=None), dict(rng=None), dict(part=None), dict(table=None)):
        rc, msg = call(**kw)
        assert rc == bad and "null pointer" in msg, (kw, rc, msg)
    rc, msg = call(K=4)
    assert rc == bad and "labels may be null only with K = 0" in msg
    for kw, text in ((dict(win=6), "win must be odd"), (dict(win=1), "win must be odd"), (dict(win=17), "win must be odd"),
                     (dict(win=9, H=7), "win=9 exceeds"), (dict(win=9, W=8), "win=9 exceeds"), (dict(K=17, lab=p), "K must be 0..16"),
                     (dict(T=65536), "T * D = 65536"), (dict(T=256, D=256), "T * D = 65536"), (dict(T=0), "bad shape")):
        rc, msg = call(**kw)
        assert rc == bad and text in msg, (kw, rc, msg)
