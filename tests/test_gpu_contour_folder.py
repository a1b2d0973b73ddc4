"""python -m cineflow.score contour end to end: two synthetic patients (4 and 12 frames -- two-digit frame numbers --, 3 slices of 24 x 20
with different point counts per slice, ED in the middle of the cine) written with tests/_score_refs.py in both layouts, plus the
reference's contour files and the ED image that carries the pixel spacing.  Every number of contour_metrics.{json,csv} and
strain_metrics.json is compared with tests/_contour_refs.py run on the same files, its chains walked one ops.sample_points call per step
on the same device: the positions are then the same bits (tests/test_gpu_contour_table.py), and what is left is fp64 arithmetic in another
order -- 1e-10 for the errors, 1e-10 relative to max(1, |value|) for the strain curves, 1e-9 for the smoothness (a variance of
quotients of second differences of those curves).  All four modes; two runs byte-identical; and the library calls per patient: one
cf_contour_track_table, one cf_contour_strain_table in mode from_ed, whatever the number of frames, and no cf_sample_points_2d."""
import collections
import csv
import json
import os

import numpy as np
import pytest

import _contour_refs as R
from _kernel_refs import ratio_line
from _score_refs import case_names, make_patient, write_tree

pytestmark = pytest.mark.gpu

PATIENTS = {"patientA": dict(seed=61, T=4, ed=1, es=3), "patientB": dict(seed=62, T=12, ed=9, es=4)}
MODES = ("from_ed", "from_ed_accumulation", "to_ed", "to_ed_accumulation")
D, H, W = 3, 24, 20
ZOOM = (1.25, 1.5)
ERR_BAR, STRAIN_BAR, SMOOTH_BAR = 1e-10, 1e-10, 1e-9


def add_ed_image(root, patient, T, ed):
    from cineflow.nifti import write_nifti
    write_nifti(os.path.join(root, "input", patient, case_names(patient, T)[ed] + "_0000.nii.gz"), np.zeros((D, H, W), np.float32),
                spacing=ZOOM + (10.0,))


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """(layout, mode) -> the files the command wrote, twice, and the documents of the restatement on the same files"""
    from cineflow import score as S
    sampler = R.device_sampler(dev)
    res = {}
    for layout in ("predict", "saver"):
        root = str(tmp_path_factory.mktemp(layout))
        for p, k in PATIENTS.items():
            out, gt, inp = write_tree(root, layout, p, make_patient(k["seed"], k["T"], D=D, H=H, W=W), k["ed"], k["es"])
            add_ed_image(root, p, k["T"], k["ed"])
            cfolder = R.write_contours(root, p, R.make_contours(k["seed"] + 100, k["T"], D, H, W))
        for mode in MODES:
            files = []
            for _ in range(2):
                if os.path.exists(os.path.join(out, "strain_metrics.json")):
                    os.remove(os.path.join(out, "strain_metrics.json"))
                S.main(["contour", "-flow", out, "-c", cfolder, "-i", inp, "--layout", layout] + (["--mode", mode] if mode != "from_ed" else []))
                names = ["contour_metrics.json", "contour_metrics.csv"] + (["strain_metrics.json"] if mode == "from_ed" else [])
                assert os.path.exists(os.path.join(out, "strain_metrics.json")) == (mode == "from_ed")
                files.append({n: _read(os.path.join(out, n)) for n in names})
            want = {}
            for p, k in PATIENTS.items():
                folder = S.patient_folders(out, layout, "Flow")[p]
                flows = [os.path.join(folder, n + ".npz") for t, n in enumerate(case_names(p, k["T"])) if t != k["ed"]]
                want[p] = R.patient_tables(flows, cfolder, p, k["ed"], ZOOM, mode, sampler)
            res[layout, mode] = dict(files=files, want=R.documents(want))
    return res


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_contour_documents_match_the_restatement(runs, layout, mode):
    from cineflow import score as S
    r = runs[layout, mode]
    assert r["files"][0] == r["files"][1], "two runs must write the same bytes"
    doc = json.loads(r["files"][0]["contour_metrics.json"])
    rows = list(csv.DictReader(r["files"][0]["contour_metrics.csv"].decode().splitlines()))
    wdoc, wrows, _ = r["want"]
    assert set(doc) == {"all", "mean", "std"} and list(doc["all"]) == sorted(PATIENTS) and list(rows[0]) == S.CONTOUR_COLUMNS
    assert len(rows) == len(wrows) == D * len(PATIENTS)
    worst, n = 0.0, 0
    for p, k in PATIENTS.items():
        assert len(doc["all"][p]) == D
        for d in range(D):
            e, w = doc["all"][p][d], wdoc["all"][p][d]
            assert set(e) == {"Name", "slice_number", "ENDO", "EPI", "RV"} and (e["Name"], e["slice_number"]) == (p, d)
            assert (rows[n]["Name"], rows[n]["slice_number"]) == (p, str(d))
            for key in R.STRUCTURES:
                assert len(e[key]) == k["T"] - 1 and not np.isnan(e[key]).any() and min(e[key]) > 0
                worst = max(worst, float(np.abs(np.array(e[key]) - np.array(w[key])).max()))           # the frame order: another order misses the bar
                assert float(rows[n][key]) == float(np.mean(e[key]))
            assert float(rows[n]["Average"]) == (float(rows[n]["ENDO"]) + float(rows[n]["EPI"]) + float(rows[n]["RV"])) / 3
            n += 1
    for key in R.STRUCTURES:
        per_slice = [np.mean(e[key]) for p in doc["all"] for e in doc["all"][p]]
        assert _same(doc["mean"][key], float(np.mean(per_slice))) and _same(doc["std"][key], float(np.std(per_slice)))
        assert abs(doc["mean"][key] - wdoc["mean"][key]) <= ERR_BAR and abs(doc["std"][key] - wdoc["std"][key]) <= ERR_BAR
    print()
    assert ratio_line("score contour (%s, %s)" % (layout, mode), worst, ERR_BAR) <= 1


@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_strain_document_matches_the_restatement(runs, layout):
    r = runs[layout, "from_ed"]
    doc = json.loads(r["files"][0]["strain_metrics.json"])
    want = r["want"][2]
    assert set(doc) == {"all", "mean"} and list(doc["all"]) == sorted(PATIENTS)
    worst = worst_smooth = 0.0
    for p, k in PATIENTS.items():
        assert len(doc["all"][p]) == D
        for d in range(D):
            e, w = doc["all"][p][d], want["all"][p][d]
            assert set(e) == {"Name", "slice_number", "radial_strain", "circ_strain", "smooth"} and (e["Name"], e["slice_number"]) == (p, d)
            for key in ("radial_strain", "circ_strain"):
                got, ref = np.array(e[key]), np.array(w[key])
                assert len(got) == k["T"] and not np.isnan(got).any()
                assert got[k["ed"]] == 0.0 and np.abs(got).max() > 1e-3                             # rolled back: the ED frame sits at its own index
                worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
            worst_smooth = max(worst_smooth, abs(e["smooth"] - w["smooth"]) / max(1.0, abs(w["smooth"])))
    per_patient = [np.mean([e["smooth"] for e in doc["all"][p]]) for p in doc["all"]]
    assert doc["mean"] == float(np.mean(per_patient))
    print()
    assert ratio_line("score contour strain (%s)" % layout, worst, STRAIN_BAR) <= 1
    assert ratio_line("score contour smoothness (%s)" % layout, worst_smooth, SMOOTH_BAR) <= 1


class Counting:
    """the ctypes library with every cf_* call counted by name (the proxy of tests/test_gpu_ssim_folder.py)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not name.startswith("cf_") or name in ("cf_last_error", "cf_version"):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


@pytest.mark.parametrize("mode", ["from_ed", "to_ed_accumulation"])
def test_library_calls_per_patient_do_not_depend_on_frames(dev, monkeypatch, tmp_path, mode):
    from cineflow import _lib, score as S
    proxy = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", proxy)
    seen = []
    for T in (4, 9):
        root = str(tmp_path / ("T%d" % T))
        out, gt, inp = write_tree(root, "predict", "patientC", make_patient(70 + T, T, D=D, H=H, W=W), 1, 2)
        add_ed_image(root, "patientC", T, 1)
        cfolder = R.write_contours(root, "patientC", R.make_contours(80 + T, T, D, H, W))
        proxy.calls.clear()
        doc = S.score_contour(out, cfolder, inp, mode=mode)
        seen.append(dict(proxy.calls))
        assert len(doc["all"]["patientC"]) == D and all(len(e["ENDO"]) == T - 1 for e in doc["all"]["patientC"])
    want = {"cf_contour_track_table": 1, "cf_contour_strain_table": 1} if mode == "from_ed" else {"cf_contour_track_table": 1}
    assert seen[0] == seen[1] == want, seen
    assert "cf_sample_points_2d" not in seen[0]
