"""cineflow.score without a GPU: which files the two sub-commands pair, in which order, for both layouts and both --gt modes; the ED / ES
rules; the ValueErrors raised before any device work; and the host functions that turn per-case rows into the json / csv documents (key
sets and column orders spelled out here, the mean blocks recomputed with numpy)."""
import csv
import json
import os
import shutil

import numpy as np
import pytest

from _score_refs import case_names, make_patient, write_tree
from cineflow import score as S

SEG_COLUMNS = ["Name", "Average_Dice", "Average_HD", "Average_ASSD", "RV_Dice", "RV_HD", "RV_ASSD", "MYO_Dice", "MYO_HD", "MYO_ASSD", "LV_Dice",
               "LV_HD", "LV_ASSD"]
JAC_COLUMNS = ["Name", "Slice nb", "Frame nb", "Temporal gradient", "Spatial gradient",
               "abs(Mean jacobian - 1)_RV", "total_RV", "negative_RV", "negative_%_RV",
               "abs(Mean jacobian - 1)_MYO", "total_MYO", "negative_MYO", "negative_%_MYO",
               "abs(Mean jacobian - 1)_LV", "total_LV", "negative_LV", "negative_%_LV",
               "abs(Mean jacobian - 1)_average", "negative_%_average", "abs(Mean jacobian - 1)", "total", "negative", "negative_%",
               "ES_negative_%", "ES_negative_%_average", "ES_negative_%_average_RV", "ES_negative_%_average_MYO", "ES_negative_%_average_LV"]
JAC_MEAN_KEYS = {"Temporal gradient", "Spatial gradient", "abs(Mean jacobian - 1)", "total_sum", "negative_sum", "negative_%", "ES_negative_%_mean",
                 "negative_%_mean", "negative_%_mean_average", "abs(Mean jacobian - 1)_average", "ES_negative_%_mean_average",
                 "negative_sum_RV", "total_sum_RV", "negative_%_RV", "negative_%_mean_RV", "abs(Mean jacobian - 1)_RV", "ES_negative_%_average_RV",
                 "negative_sum_MYO", "total_sum_MYO", "negative_%_MYO", "negative_%_mean_MYO", "abs(Mean jacobian - 1)_MYO", "ES_negative_%_average_MYO",
                 "negative_sum_LV", "total_sum_LV", "negative_%_LV", "negative_%_mean_LV", "abs(Mean jacobian - 1)_LV", "ES_negative_%_average_LV"}


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """patientA: 12 frames (two-digit frame numbers sort after one-digit ones only numerically), ED 2, ES 5; in both layouts"""
    data = make_patient(3, 12, D=2, H=10, W=8)
    out = {}
    for layout in ("predict", "saver"):
        root = str(tmp_path_factory.mktemp(layout))
        out[layout] = write_tree(root, layout, "patientA", data, ed=2, es=5)
    return out


# ------------------------------------------------------------------------------------------------ discovery
@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_patient_folders_and_sorting(trees, layout):
    out, gt, inp = trees[layout]
    reg = S.patient_folders(out, layout, "Registered")
    flow = S.patient_folders(out, layout, "Flow")
    assert list(reg) == list(flow) == ["patientA"]
    if layout == "predict":
        assert reg["patientA"] == os.path.join(out, "patientA", "Registered") and flow["patientA"] == os.path.join(out, "patientA", "Flow")
    else:
        assert reg["patientA"] == os.path.join(out, "Postprocessed", "Registered", "patientA", "temp_allClasses")
        assert flow["patientA"] == os.path.join(out, "Postprocessed", "Flow", "patientA")
    names = case_names("patientA", 12)
    want = names if layout == "predict" else names[:2] + names[3:]                  # the saver layout has no ED files
    assert S.sorted_cases(reg["patientA"], ".nii.gz") == want
    assert S.sorted_cases(flow["patientA"], ".npz") == want
    # the order is numeric on the last two characters, not lexicographic on the name
    os.makedirs(os.path.join(out, "scratch"), exist_ok=True)
    for n in ("b_x10.nii.gz", "a_x09.nii.gz", "c_x02.nii.gz", "notes.txt"):
        open(os.path.join(out, "scratch", n), "w").close()
    assert S.sorted_cases(os.path.join(out, "scratch"), ".nii.gz") == ["c_x02", "a_x09", "b_x10"]
    with pytest.raises(ValueError, match="layout"):
        S.patient_folders(out, "flat", "Registered")


def test_saver_layout_without_filtered_folder_falls_back(tmp_path):
    d = tmp_path / "Postprocessed" / "Registered" / "p1"
    d.mkdir(parents=True)
    assert S.patient_folders(str(tmp_path), "saver", "Registered") == {"p1": str(d)}
    with pytest.raises(ValueError, match="Postprocessed/Flow"):
        S.patient_folders(str(tmp_path), "saver", "Flow")


def test_ed_es_rules(trees):
    out, gt, inp = trees["predict"]
    assert S.ed_es_indices(inp, "patientA") == (2, 5)
    assert S.ed_es_indices(None, "patientA") == (0, 0)
    assert S.reference_name("patientA_frame07", "frame", 2) == "patientA_frame07"
    assert S.reference_name("patientA_frame07", "ed", 2) == "patientA_frame03"       # frame digits <- ed_index + 1, zero-filled
    assert S.reference_name("patientA_frame07", "ed", 11) == "patientA_frame12"
    with pytest.raises(ValueError, match="--gt"):
        S.reference_name("patientA_frame07", "es", 0)


@pytest.mark.parametrize("layout", ["predict", "saver"])
@pytest.mark.parametrize("gt_mode", ["frame", "ed"])
def test_segmentation_pairing(trees, layout, gt_mode, tmp_path):
    out, gt, inp = trees[layout]
    folder = S.patient_folders(out, layout, "Registered")["patientA"]
    names = case_names("patientA", 12)
    present = names if layout == "predict" else names[:2] + names[3:]
    cases = S.pair_segmentation_cases(folder, gt, gt_mode, 2)
    assert [c.name for c in cases] == present and [c.frame for c in cases] == [int(n[-2:]) for n in present]
    for c in cases:
        assert c.path == os.path.join(folder, c.name + ".nii.gz")
        assert c.other == os.path.join(gt, (c.name if gt_mode == "frame" else "patientA_frame03") + ".nii.gz")
    # cases without a GT file are skipped: a GT folder that holds frames 3 and 7 only
    sparse = tmp_path / "gt"
    sparse.mkdir()
    for n in (names[2], names[6]):
        shutil.copyfile(os.path.join(gt, n + ".nii.gz"), str(sparse / (n + ".nii.gz")))
    got = [c.name for c in S.pair_segmentation_cases(folder, str(sparse), gt_mode, 2)]
    if gt_mode == "ed":
        assert got == present                                                       # every frame is scored against frame 3's GT
    else:
        assert got == [n for n in (names[2], names[6]) if n in present]
    assert S.pair_segmentation_cases(folder, str(sparse), "ed", 0) == []             # frame 1's GT is not there: nothing to score


@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_jacobian_pairing_and_errors(trees, layout, tmp_path):
    out, gt, inp = trees[layout]
    folder = S.patient_folders(out, layout, "Flow")["patientA"]
    names = case_names("patientA", 12)
    no_ed = names[:2] + names[3:]
    # the ED frame's file (frame number ed_index + 1) is left out where the layout writes one; an unknown ED leaves everything in
    assert [c.name for c in S.pair_jacobian_cases(folder, gt, "patientA", 2)] == no_ed
    assert [c.name for c in S.pair_jacobian_cases(folder, gt, "patientA", None)] == (names if layout == "predict" else no_ed)
    # labels flat (gt), per patient (the saver's Segmentation folder) or <patient>/Segmentation (the predict output itself)
    own = out if layout == "predict" else os.path.join(out, "Postprocessed", "Segmentation")
    cases = S.pair_jacobian_cases(folder, own, "patientA", 2)
    sub = ("patientA", "Segmentation") if layout == "predict" else ("patientA",)
    assert [c.other for c in cases] == [os.path.join(own, *sub, n + ".nii.gz") for n in no_ed]
    assert [c.other for c in S.pair_jacobian_cases(folder, gt, "patientA", 2)] == [os.path.join(gt, n + ".nii.gz") for n in no_ed]
    # a missing label volume names the case
    sparse = tmp_path / "labels"
    sparse.mkdir()
    for n in no_ed[:-1]:
        shutil.copyfile(os.path.join(gt, n + ".nii.gz"), str(sparse / (n + ".nii.gz")))
    with pytest.raises(ValueError, match="patientA_frame12"):
        S.pair_jacobian_cases(folder, str(sparse), "patientA", 2)
    # a mis-shaped one too (read from the headers: [Z, Y, X] against the flow's [H, W, D])
    from cineflow.nifti import write_nifti
    write_nifti(str(sparse / (no_ed[-1] + ".nii.gz")), np.zeros((2, 10, 9), np.uint8))
    with pytest.raises(ValueError, match=r"patientA_frame12.*\(2, 10, 9\)"):
        S.pair_jacobian_cases(folder, str(sparse), "patientA", 2)


def test_header_shapes(trees):
    out, gt, inp = trees["predict"]
    assert S._nifti_shape(os.path.join(gt, "patientA_frame01.nii.gz")) == (2, 10, 8)
    assert S._npz_shape(os.path.join(out, "patientA", "Flow", "patientA_frame01.npz"), "flow") == (10, 8, 2, 2)


def test_readers_check_shapes_and_keep_structures_only(trees, tmp_path):
    out, gt, inp = trees["predict"]
    from cineflow.nifti import write_nifti
    a = np.array([[[0, 1, 2, 3, 4, 7]]], np.int16)
    write_nifti(str(tmp_path / "x_01.nii.gz"), a, spacing=(1.5, 2.5, 8.0))
    write_nifti(str(tmp_path / "y_01.nii.gz"), a.astype(np.float32), spacing=(1.5, 2.5, 8.0))
    t, r, sp = S._read_seg_case(S.Case("x_01", 1, str(tmp_path / "x_01.nii.gz"), str(tmp_path / "y_01.nii.gz")))
    assert t.dtype == r.dtype == np.uint8 and t.tolist() == r.tolist() == [[[0, 1, 2, 3, 0, 0]]]
    assert sp == (8.0, 2.5, 1.5)                                                     # the GT header's zooms in array order (z, y, x)
    write_nifti(str(tmp_path / "z_01.nii.gz"), np.zeros((1, 2, 3), np.uint8))
    with pytest.raises(ValueError, match="x_01"):
        S._read_seg_case(S.Case("x_01", 1, str(tmp_path / "x_01.nii.gz"), str(tmp_path / "z_01.nii.gz")))
    flow, lab = S._read_jacobian_case(S.Case("c", 1, os.path.join(out, "patientA", "Flow", "patientA_frame01.npz"), os.path.join(gt, "patientA_frame01.nii.gz")))
    assert flow.shape == (10, 8, 2, 2) and flow.dtype == np.float32 and lab.shape == (10, 8, 2)


# ------------------------------------------------------------------------------------------------ table assembly
def _seg_case(patient, name, is_es, values):
    it = iter(values)
    return {"patient": patient, "name": name, "test": "/p/" + name, "reference": "/g/" + name, "is_es": is_es,
            "scores": {s: {m: next(it) for m in ("Dice", "HD", "ASSD")} for s in ("RV", "MYO", "LV")}}


def test_segmentation_tables_from_rows(tmp_path):
    nan = float("nan")
    cases = [_seg_case("p1", "p1_frame01", False, [0.9, 2.0, 0.5, 0.8, 3.0, 0.7, 0.95, 1.0, 0.25]),
             _seg_case("p1", "p1_frame02", True, [0.7, 4.0, 1.5, nan, nan, nan, 0.85, 2.0, 0.75]),
             _seg_case("p2", "p2_frame01", True, [0.5, 6.0, 2.5, 0.6, 5.0, 1.7, 0.75, 3.0, 1.25])]
    doc, rows, es_rows = S.segmentation_tables(cases)
    assert set(doc) == {"all", "mean", "std"} and list(doc["all"]) == ["p1", "p2"] and [len(v) for v in doc["all"].values()] == [2, 1]
    for entry in doc["all"]["p1"] + doc["all"]["p2"]:
        assert set(entry) == {"RV", "MYO", "LV", "test", "reference"}
        assert all(set(entry[s]) == {"Dice", "HD", "ASSD"} for s in ("RV", "MYO", "LV"))
    assert doc["all"]["p1"][1]["test"] == "/p/p1_frame02" and doc["all"]["p1"][1]["reference"] == "/g/p1_frame02"
    assert set(doc["mean"]) == set(doc["std"]) == {"RV", "MYO", "LV"}
    # nanmean skips the NaN case, std does not
    assert doc["mean"]["RV"]["Dice"] == float(np.nanmean(np.array([0.9, 0.7, 0.5]))) and doc["std"]["RV"]["HD"] == float(np.std(np.array([2.0, 4.0, 6.0])))
    assert doc["mean"]["MYO"]["HD"] == float(np.nanmean(np.array([3.0, nan, 5.0]))) == 4.0 and np.isnan(doc["std"]["MYO"]["HD"])
    assert [list(r) for r in rows] == [SEG_COLUMNS] * 3 and [r["Name"] for r in rows] == ["p1_frame01", "p1_frame02", "p2_frame01"]
    assert rows[0]["Average_Dice"] == (0.9 + 0.8 + 0.95) / 3 and rows[0]["Average_HD"] == (2.0 + 3.0 + 1.0) / 3 and rows[0]["LV_ASSD"] == 0.25
    assert np.isnan(rows[1]["Average_ASSD"]) and rows[1]["RV_HD"] == 4.0
    assert [r["Name"] for r in es_rows] == ["p1_frame02", "p2_frame01"]
    S.save_json(doc, str(tmp_path / "m.json"))
    S.write_csv(str(tmp_path / "m.csv"), S.SEG_COLUMNS, rows)
    text = open(str(tmp_path / "m.json")).read()
    assert text.startswith('{\n    "all": {\n        "p1": [') and "NaN" in text           # sort_keys, indent 4, NaN as json.dump writes it
    assert json.loads(text)["mean"]["LV"]["Dice"] == doc["mean"]["LV"]["Dice"]
    with open(str(tmp_path / "m.csv"), newline="") as f:
        read = list(csv.reader(f))
    assert read[0] == SEG_COLUMNS and len(read) == 4 and read[2][0] == "p1_frame02" and read[2][8] == "nan"
    # no case at all: header-only tables, NaN means
    doc, rows, es_rows = S.segmentation_tables([])
    assert doc["all"] == {} and rows == [] and np.isnan(doc["mean"]["RV"]["Dice"])


def _stats(rng, absent=None):
    st = {"Temporal gradient": float(rng.random()), "Spatial gradient": float(rng.random())}
    for k in ("RV", "MYO", "LV"):
        total = 0.0 if k == absent else float(rng.integers(5, 50))
        neg = 0.0 if k == absent else float(rng.integers(0, 5))
        st["abs(Mean jacobian - 1)_" + k] = float("nan") if k == absent else float(rng.random())
        st["total_" + k], st["negative_" + k] = total, neg
        st["negative_%_" + k] = float("nan") if k == absent else neg / total * 100
    st["abs(Mean jacobian - 1)_average"] = sum(st["abs(Mean jacobian - 1)_" + k] for k in ("RV", "MYO", "LV")) / 3
    st["negative_%_average"] = sum(st["negative_%_" + k] for k in ("RV", "MYO", "LV")) / 3
    st["abs(Mean jacobian - 1)"], st["total"], st["negative"] = float(rng.random()), 80.0, float(rng.integers(0, 9))
    st["negative_%"] = st["negative"] / 80.0 * 100
    return st


def test_jacobian_tables_from_rows():
    rng = np.random.default_rng(5)
    names = ["p_frame01", "p_frame02", "p_frame04"]
    stats = [_stats(rng) for _ in range(6)]                                          # 2 slices x 3 frames, slices outermost
    rows = S.jacobian_rows(names, stats, 2)
    assert [list(r) for r in rows] == [JAC_COLUMNS] * 6
    assert [(r["Name"], r["Slice nb"], r["Frame nb"]) for r in rows] == [(n, float(d), float(t)) for d in range(2) for t, n in enumerate(names)]
    for i, r in enumerate(rows):
        if i % 3 == 2:                                                               # the ES frame's rows carry their own figures
            assert (r["ES_negative_%"], r["ES_negative_%_average"]) == (r["negative_%"], r["negative_%_average"])
            assert [r["ES_negative_%_average_" + k] for k in ("RV", "MYO", "LV")] == [r["negative_%_" + k] for k in ("RV", "MYO", "LV")]
        else:
            assert all(np.isnan(r[k]) for k in JAC_COLUMNS[-5:])
    assert all(np.isnan(r["ES_negative_%"]) for r in S.jacobian_rows(names, stats, None))
    doc = S.jacobian_tables(rows)
    assert set(doc) == {"all", "mean"} and set(doc["mean"]) == JAC_MEAN_KEYS and len(doc["all"]) == 6
    col = lambda k: np.array([r[k] for r in rows])                                   # noqa: E731
    m = doc["mean"]
    assert m["Temporal gradient"] == col("Temporal gradient").mean() and m["Spatial gradient"] == col("Spatial gradient").mean()
    assert m["total_sum"] == col("total").sum() == 480.0 and m["negative_sum"] == col("negative").sum()
    assert m["negative_%"] == col("negative").sum() / col("total").sum() * 100 and m["negative_%_mean"] == col("negative_%").mean()
    assert m["abs(Mean jacobian - 1)"] == col("abs(Mean jacobian - 1)").mean()
    assert m["abs(Mean jacobian - 1)_average"] == col("abs(Mean jacobian - 1)_average").mean()
    assert m["negative_%_mean_average"] == col("negative_%_average").mean()
    assert m["ES_negative_%_mean"] == np.nanmean(col("ES_negative_%")) == np.mean([rows[2]["negative_%"], rows[5]["negative_%"]])
    assert m["ES_negative_%_mean_average"] == np.nanmean(col("ES_negative_%_average"))
    for k in ("RV", "MYO", "LV"):
        assert m["negative_sum_" + k] == col("negative_" + k).sum() and m["total_sum_" + k] == col("total_" + k).sum()
        assert m["negative_%_" + k] == col("negative_" + k).sum() / col("total_" + k).sum() * 100
        assert m["negative_%_mean_" + k] == col("negative_%_" + k).mean() and m["abs(Mean jacobian - 1)_" + k] == col("abs(Mean jacobian - 1)_" + k).mean()
        assert np.isnan(m["ES_negative_%_average_" + k])                             # a plain mean over a column that is NaN off the ES frame
    # a frame without a structure: its NaN entries make the plain means NaN, the sums stay
    rows2 = S.jacobian_rows(names, [_stats(rng, absent="MYO" if i == 1 else None) for i in range(3)], 0)
    m2 = S.jacobian_tables(rows2)["mean"]
    assert np.isnan(m2["negative_%_mean_MYO"]) and np.isnan(m2["abs(Mean jacobian - 1)_average"]) and not np.isnan(m2["negative_%_MYO"])
    assert not np.isnan(m2["negative_%_mean_RV"]) and m2["ES_negative_%_mean"] == rows2[0]["negative_%"]
    json.dumps(S.jacobian_tables(rows))                                              # plain floats throughout


def test_cli_parser():
    p = S.build_parser()
    a = p.parse_args(["seg", "-pred", "P", "-ref", "G", "--gt", "ed", "--layout", "saver", "-i", "I"])
    assert (a.command, a.pred, a.ref, a.gt, a.layout, a.i) == ("seg", "P", "G", "ed", "saver", "I")
    a = p.parse_args(["jacobian", "-flow", "F", "-l", "L"])
    assert (a.command, a.flow, a.l, a.layout, a.i) == ("jacobian", "F", "L", "predict", None)
    a = p.parse_args(["seg", "-pred", "P", "-ref", "G"])
    assert (a.gt, a.layout, a.i) == ("frame", "predict", None)
