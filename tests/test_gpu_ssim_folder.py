"""python -m cineflow.score ssim end to end: two synthetic patients (4 and 12 frames -- two-digit frame numbers --, 3 slices of 24 x 20,
ES != ED) written with tests/_score_refs.py in both layouts plus their <case>_0000.nii.gz images; with and without -l.  Every number of
the json and csv files is compared with the per-pair device path restated here -- ops.warp_bilinear, then
metrics.structural_similarity(full=True) with data_range = max - min of the registered slice, then the three mask means -- at 1e-10 for
whole-slice scores and 1e-9 for structure scores: both paths use the same device warp, so the SSIM arithmetic is the only difference.
Also: the frame order (rotated to start after ED), the ES columns, the `mean` blocks recomputed with numpy, two runs byte-identical, and
two library calls per patient whatever the number of frames."""
import collections
import csv
import json
import os

import numpy as np
import pytest
import torch

from _kernel_refs import ratio_line
from _score_refs import NAMES, case_names, make_patient, write_tree

pytestmark = pytest.mark.gpu

PATIENTS = {"patientA": dict(seed=31, T=4, ed=1, es=3), "patientB": dict(seed=32, T=12, ed=9, es=4)}
PLAIN_FILES = ("ssim_metrics.json", "ssim_metrics.csv")
ALL_FILES = ("ssim_metrics_all.json", "ssim_metrics_all.csv")
KEYS = ("SSIM_mean", "SSIM_rv", "SSIM_myo", "SSIM_lv", "SSIM_whole")
WHOLE_BAR, STRUCT_BAR = 1e-10, 1e-9


def make_images(seed, T, D=3, H=24, W=20):
    """float32 [T, D, H, W] in file order (Z, Y, X): one N(300, 40^2) figure with per-frame noise"""
    rng = np.random.default_rng(seed)
    base = rng.normal(300.0, 40.0, size=(D, H, W))
    return (base[None] + rng.normal(0.0, 10.0, size=(T, D, H, W))).astype(np.float32)


def add_images(root, patient, images):
    from cineflow.nifti import write_nifti
    for name, img in zip(case_names(patient, len(images)), images):
        write_nifti(os.path.join(root, "input", patient, name + "_0000.nii.gz"), img)


def _bytes(folder, names):
    out = {}
    for n in names:
        with open(os.path.join(folder, n), "rb") as f:
            out[n] = f.read()
    return out


def per_pair(dev, images, flow, labels, ed):
    """-> {frame position t != ed: [D] dicts of the five scores}: one call chain per (frame, slice)"""
    from cineflow import metrics, ops
    T, D = images.shape[:2]
    res = {}
    for t in range(T):
        if t == ed:
            continue
        res[t] = []
        for d in range(D):
            f = torch.from_numpy(np.ascontiguousarray(flow[t, :, :, d].transpose(2, 0, 1)))[None].to(dev)
            m = torch.from_numpy(images[t, d])[None, None].to(dev)
            reg = ops.warp_bilinear(f, m)[0, 0].cpu().numpy()
            score, smap = metrics.structural_similarity(images[ed, d].astype(np.float64), reg, win_size=7, data_range=reg.max() - reg.min(), full=True)
            per = [float(smap[labels[d] == k].mean()) for k in (1, 2, 3)]
            row = {"SSIM_whole": score, "SSIM_mean": sum(per) / 3}
            row.update({"SSIM_" + n.lower(): v for n, v in zip(NAMES, per)})
            res[t].append(row)
    return res


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """layout -> the data, the reference scores and the files of the runs: without -l, then twice with -l"""
    from cineflow import score as S
    data = {p: make_patient(k["seed"], k["T"]) for p, k in PATIENTS.items()}
    images = {p: make_images(k["seed"] + 100, k["T"]) for p, k in PATIENTS.items()}
    want = {p: per_pair(dev, images[p], data[p]["flow"], data[p]["gt"][k["ed"]], k["ed"]) for p, k in PATIENTS.items()}
    res = {}
    for layout in ("predict", "saver"):
        root = str(tmp_path_factory.mktemp(layout))
        for p, k in PATIENTS.items():
            out, gt, inp = write_tree(root, layout, p, data[p], k["ed"], k["es"])
            add_images(root, p, images[p])
        labels = out if layout == "predict" else os.path.join(out, "Postprocessed", "Segmentation")
        S.main(["ssim", "-flow", out, "-i", inp, "--layout", layout])
        assert not any(os.path.exists(os.path.join(out, n)) for n in ALL_FILES), "without -l only ssim_metrics.* are written"
        plain = _bytes(out, PLAIN_FILES)
        both = []
        for _ in range(2):
            S.main(["ssim", "-flow", out, "-i", inp, "-l", labels, "--layout", layout])
            both.append(_bytes(out, PLAIN_FILES + ALL_FILES))
        res[layout] = dict(want=want, plain=plain, both=both)
    return res


def _order(k):
    """frame positions in the documents' order: by frame number, starting with the first frame after ED"""
    return [t for t in range(k["T"]) if t > k["ed"]] + [t for t in range(k["T"]) if t < k["ed"]]


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("layout", ["predict", "saver"])
def test_ssim_tables_match_the_per_pair_path(runs, layout):
    from cineflow import score as S
    r = runs[layout]
    assert r["both"][0] == r["both"][1], "two runs must write the same bytes"
    assert {n: r["both"][0][n] for n in PLAIN_FILES} == r["plain"], "-l does not change ssim_metrics.*"
    doc = json.loads(r["plain"]["ssim_metrics.json"])
    doc_all = json.loads(r["both"][0]["ssim_metrics_all.json"])
    rows = list(csv.DictReader(r["plain"]["ssim_metrics.csv"].decode().splitlines()))
    rows_all = list(csv.DictReader(r["both"][0]["ssim_metrics_all.csv"].decode().splitlines()))
    assert list(rows[0]) == S.SSIM_COLUMNS and list(rows_all[0]) == S.SSIM_ALL_COLUMNS
    assert len(doc["all"]) == len(doc_all["all"]) == len(rows) == len(rows_all) == 3 * len(PATIENTS)
    worst_w = worst_s = 0.0
    n = 0
    for p, k in PATIENTS.items():                                  # patients sorted, slices inside
        order, want = _order(k), r["want"][p]
        assert len(order) == k["T"] - 1 and k["es"] in order
        for d in range(3):
            e, ea = doc["all"][n], doc_all["all"][n]
            assert set(e) == set(S.SSIM_COLUMNS) and set(ea) == set(S.SSIM_ALL_COLUMNS)
            assert (e["Name"], e["slice_number"]) == (p, d) == (ea["Name"], ea["slice_number"])
            assert (rows[n]["Name"], rows[n]["slice_number"]) == (p, str(d)) == (rows_all[n]["Name"], rows_all[n]["slice_number"])
            assert len(e["SSIM"]) == len(order) and e["SSIM"] == ea["SSIM_whole"]
            for key in KEYS:
                assert len(ea[key]) == len(order)
                for got, t in zip(ea[key], order):                 # the frame order: a rotated or unrotated list would miss the bars
                    w = want[t][d][key]
                    assert not np.isnan(w) and not np.isnan(got), (p, d, t, key)
                    if key == "SSIM_whole":
                        worst_w = max(worst_w, abs(got - w))
                    else:
                        worst_s = max(worst_s, abs(got - w))
                assert ea["ES_" + key] == ea[key][order.index(k["es"])]
                assert float(rows_all[n][key]) == float(np.mean(ea[key])) and float(rows_all[n]["ES_" + key]) == ea["ES_" + key]
            assert float(rows[n]["SSIM"]) == float(np.mean(e["SSIM"]))
            n += 1
    assert _same(doc["mean"], float(np.mean([np.mean(e["SSIM"]) for e in doc["all"]])))
    assert _same(doc_all["mean"], float(np.mean([np.mean(e["SSIM_mean"]) for e in doc_all["all"]])))
    assert not np.isnan(doc["mean"]) and not np.isnan(doc_all["mean"])
    print()
    assert ratio_line("score ssim (%s) whole" % layout, worst_w, WHOLE_BAR) <= 1
    assert ratio_line("score ssim (%s) structures" % layout, worst_s, STRUCT_BAR) <= 1


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


def test_library_calls_per_patient_do_not_depend_on_frames(dev, monkeypatch, tmp_path):
    from cineflow import _lib, score as S
    proxy = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", proxy)
    seen = []
    for T in (4, 12):
        root = str(tmp_path / ("T%d" % T))
        out, gt, inp = write_tree(root, "predict", "patientC", make_patient(40 + T, T), 1, 2)
        add_images(root, "patientC", make_images(50 + T, T))
        proxy.calls.clear()
        doc = S.score_ssim(out, inp, out)
        seen.append(dict(proxy.calls))
        assert len(doc["all"]) == 3 and all(len(e["SSIM"]) == T - 1 for e in doc["all"])
    assert seen[0] == seen[1] == {"cf_warp_bilinear_2d": 1, "cf_cine_ssim_table": 1}, seen
