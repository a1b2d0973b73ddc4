"""python -m cineflow.score end to end: two synthetic patients (4 and 5 frames, 3 slices of 24 x 20, ES != ED) written with cineflow.nifti
and np.savez in both layouts; both sub-commands; every number of the json and csv files against rows built from the oracle's per-frame
functions (tests/_score_refs.py) at the bars of tests/test_gpu_score_kernels.py; two runs give byte-identical files; and the number of
library calls per patient does not depend on the number of frames or classes."""
import collections
import csv
import json
import os

import numpy as np
import pytest

from _score_refs import NAMES, case_names, check_jacobian_row, jacobian_rows, make_patient, seg_scores, write_tree

pytestmark = pytest.mark.gpu

PATIENTS = {"patientA": dict(seed=11, T=4, ed=1, es=3), "patientB": dict(seed=12, T=5, ed=0, es=2)}
SPACING = (1.25, 1.25, 10.0)                     # the header's (x, y, z); the arrays are [Z, Y, X]
ARRAY_SPACING = (10.0, 1.25, 1.25)
GT_MODE = {"predict": "frame", "saver": "ed"}
SEG_FILES = ("segmentation_metrics.json", "segmentation_metrics.csv", "segmentation_metrics_es.csv")
JAC_FILES = ("jacobian.json", "jacobian_metrics.csv")


def _bytes(folder, names):
    out = {}
    for n in names:
        with open(os.path.join(folder, n), "rb") as f:
            out[n] = f.read()
    return out


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """layout -> (data, folders, the files of two runs of each sub-command)"""
    from cineflow import score as S
    data = {p: make_patient(k["seed"], k["T"]) for p, k in PATIENTS.items()}
    res = {}
    for layout in ("predict", "saver"):
        root = str(tmp_path_factory.mktemp(layout))
        for p, k in PATIENTS.items():
            out, gt, inp = write_tree(root, layout, p, data[p], k["ed"], k["es"], SPACING)
        labels = out if layout == "predict" else os.path.join(out, "Postprocessed", "Segmentation")
        seg, jac = [], []
        for _ in range(2):
            S.main(["seg", "-pred", out, "-ref", gt, "-i", inp, "--gt", GT_MODE[layout], "--layout", layout])
            seg.append(_bytes(out, SEG_FILES))
            S.main(["jacobian", "-flow", out, "-l", labels, "-i", inp, "--layout", layout])
            jac.append(_bytes(out, JAC_FILES))
        res[layout] = dict(data=data, out=out, gt=gt, seg=seg, jac=jac)
    return res


def _frames(layout, k):
    """frame positions that have Registered / Flow files to score"""
    return [t for t in range(k["T"]) if not (layout == "saver" and t == k["ed"])]


def _close(got, want, bar=1e-12):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= bar


@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_segmentation_tables_match_the_oracle(runs, layout):
    r = runs[layout]
    assert r["seg"][0] == r["seg"][1], "two runs must write the same bytes"
    doc = json.loads(r["seg"][0]["segmentation_metrics.json"])
    rows = list(csv.DictReader(r["seg"][0]["segmentation_metrics.csv"].decode().splitlines()))
    es_rows = list(csv.DictReader(r["seg"][0]["segmentation_metrics_es.csv"].decode().splitlines()))
    assert list(doc["all"]) == list(PATIENTS)
    flat, want_names, want_es = [], [], []
    for p, k in PATIENTS.items():
        names, d = case_names(p, k["T"]), r["data"][p]
        ts = _frames(layout, k)
        assert len(doc["all"][p]) == len(ts)
        for entry, t in zip(doc["all"][p], ts):
            ref_t = t if GT_MODE[layout] == "frame" else k["ed"]
            want = seg_scores(d["reg"][t], d["gt"][ref_t], ARRAY_SPACING)
            assert os.path.basename(entry["test"]) == names[t] + ".nii.gz" and os.path.basename(entry["reference"]) == names[ref_t] + ".nii.gz"
            assert "temp_allClasses" in entry["test"] or layout == "predict"
            for s in NAMES:
                for m in ("Dice", "HD", "ASSD"):
                    assert not np.isnan(want[s][m]) and _close(entry[s][m], want[s][m]), (p, t, s, m, entry[s][m], want[s][m])
            flat.append(want)
            want_names.append(names[t])
            if t == k["es"]:
                want_es.append(names[t])
    for s in NAMES:
        for m in ("Dice", "HD", "ASSD"):
            col = np.array([w[s][m] for w in flat])
            assert _close(doc["mean"][s][m], np.nanmean(col)) and _close(doc["std"][s][m], np.std(col))
    assert [x["Name"] for x in rows] == want_names and [x["Name"] for x in es_rows] == want_es and len(want_es) == 2
    for row, want in zip(rows, flat):
        for m in ("Dice", "HD", "ASSD"):
            assert _close(float(row["Average_" + m]), sum(want[s][m] for s in NAMES) / 3)
            for s in NAMES:
                assert _close(float(row["%s_%s" % (s, m)]), want[s][m])
    assert es_rows[0] == next(x for x in rows if x["Name"] == want_es[0])


@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_jacobian_tables_match_the_oracle(runs, layout):
    from cineflow import score as S
    r = runs[layout]
    assert r["jac"][0] == r["jac"][1], "two runs must write the same bytes"
    doc = json.loads(r["jac"][0]["jacobian.json"])
    rows = list(csv.DictReader(r["jac"][0]["jacobian_metrics.csv"].decode().splitlines()))
    got = iter(doc["all"])
    n = 0
    worst = collections.Counter()
    for p, k in PATIENTS.items():
        names, d = case_names(p, k["T"]), r["data"][p]
        ts = [t for t in range(k["T"]) if t != k["ed"]]                              # the ED frame's flow is left out in both layouts
        want, near = jacobian_rows(d["flow"][ts], d["gt"][ts].transpose(0, 2, 3, 1))
        assert max(near) <= 2
        for i, w in enumerate(want):
            g = next(got)
            z, pos = divmod(i, len(ts))
            assert (g["Name"], g["Slice nb"], g["Frame nb"]) == (names[ts[pos]], float(z), float(pos))
            for kind, v in check_jacobian_row(g, w, near[i], "%s %s" % (p, g["Name"])).items():
                worst[kind] = max(worst[kind], v)
            es = ts[pos] == k["es"]
            for es_key, key in S.JACOBIAN_ES_KEYS:
                assert (g[es_key] == g[key]) if es else np.isnan(g[es_key]), (p, g["Name"], es_key)
            assert set(rows[n]) == set(g)
            assert rows[n]["Name"] == g["Name"] and _close(float(rows[n]["negative_%"]), g["negative_%"]) and _close(float(rows[n]["total_LV"]), g["total_LV"])
            n += 1
    assert n == len(doc["all"]) == len(rows) == 3 * (3 + 4)
    print("\n  jacobian rows (%s): worst %s" % (layout, dict(worst)))
    again = S.jacobian_tables(doc["all"])["mean"]
    assert set(again) == set(doc["mean"])
    for key, v in again.items():
        assert _close(doc["mean"][key], v, 0.0), key
    assert doc["mean"]["total_sum"] == 21 * 24 * 20 and np.isnan(doc["mean"]["ES_negative_%_average_LV"]) and not np.isnan(doc["mean"]["ES_negative_%_mean"])


class Counting:
    """the ctypes library with every cf_* call counted by name"""

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


def test_library_calls_per_patient_do_not_depend_on_frames_or_classes(dev, monkeypatch):
    from cineflow import _lib, metrics, score as S
    proxy = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", proxy)
    seen = []
    for T, classes in ((2, (2, 3)), (5, (1, 2, 3))):
        d = make_patient(20 + T, T, classes=classes)
        proxy.calls.clear()
        scores = S.score_segmentation_patient([(d["reg"][t], d["gt"][t], ARRAY_SPACING) for t in range(T)])
        seg_calls = dict(proxy.calls)
        proxy.calls.clear()
        table = metrics.cine_jacobian_table(d["flow"], d["gt"].transpose(0, 2, 3, 1))
        seen.append((seg_calls, dict(proxy.calls)))
        assert len(scores) == T and len(table) == 3 * T
        assert np.isnan(scores[0]["RV"]["Dice"]) == (1 not in classes) and not np.isnan(scores[0]["LV"]["HD"])
    assert seen[0] == seen[1] == ({"cf_label_surface_count": 1, "cf_label_surface_table": 1}, {"cf_flow_regularity_table": 1}), seen
