"""cineflow.evaluation on the EDT route: a seeded folder of three (6, 24, 20) cases with labels 1-3, scored with surface="pairs" and with
surface="edt".  The spacing is dyadic, so every distance is the same number on both routes: the overlap metrics, HD and HD95 must be
identical, and the mean distances agree to 1e-15 relative (the pairs route sums the sorted vector on the host, the EDT route sums on
the device in raster order).  The library handle is wrapped to see which calls each route makes."""
import json
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (6, 24, 20)
ITK_SPACING = (0.78125, 0.78125, 2.5)            # x, y, z: voxel spacing (2.5, 0.78125, 0.78125) on the array axes
MEANS = ("Avg. Symmetric Surface Distance", "Avg. Surface Distance")


def make_folders(root):
    from scipy.ndimage import gaussian_filter
    from cineflow.nifti import write_nifti
    gt, pred = os.path.join(root, "gt"), os.path.join(root, "pred")
    os.makedirs(gt), os.makedirs(pred)
    for i in range(3):
        rng = np.random.default_rng(100 + i)
        f = gaussian_filter(rng.random(SHAPE), 1.5)
        ref = np.digitize(f, np.quantile(f, [0.4, 0.6, 0.8])).astype(np.uint8)                # labels 0..3, each in every slice range
        noise = rng.random(SHAPE) < 0.1
        test = np.where(noise, rng.integers(0, 4, SHAPE), ref).astype(np.uint8)
        assert all(((ref[2:] == c).any() and (test[2:] == c).any()) for c in (1, 2, 3))
        name = "case_%02d.nii.gz" % i
        write_nifti(os.path.join(gt, name), ref, spacing=ITK_SPACING)
        write_nifti(os.path.join(pred, name), test, spacing=ITK_SPACING)
    return gt, pred


class CountingLib:
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


def run(gt, pred, monkeypatch=None, **kw):
    from cineflow import evaluation as E
    from cineflow import metrics as M
    counter = None
    if monkeypatch is not None:
        counter = CountingLib(M.lib())
        monkeypatch.setattr(M, "lib", lambda: counter)
        monkeypatch.setattr(E, "lib", lambda: counter)
    E.evaluate_folder(gt, pred, [1, 2, 3], **kw)
    if monkeypatch is not None:
        monkeypatch.undo()
    raw = open(os.path.join(pred, "summary.json"), "rb").read()
    return json.loads(raw)["results"], raw, (counter.calls if counter else None)


def same(a, b, path=""):
    """two `results` trees: every number identical, the mean distances to 1e-15 relative"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, float) and path.rsplit("/", 1)[-1] in MEANS:
        print("%s: %.17g vs %.17g" % (path, a, b))
        assert abs(a - b) <= 1e-15 * abs(b), (path, a, b)
    else:
        assert a == b or (a != a and b != b), (path, a, b)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    return make_folders(str(tmp_path_factory.mktemp("edt_eval")))


@pytest.fixture(scope="module")
def pairs_results(folders, dev):
    return run(*folders, surface="pairs")[0]


def test_edt_route_writes_the_summary_of_the_pairs_route(dev, folders, pairs_results, monkeypatch):
    default = run(*folders)[0]                                           # the default route stays on pairs at this size: the same document
    same(default, pairs_results)
    edt, _, calls = run(*folders, monkeypatch=monkeypatch, surface="edt")
    same(edt, pairs_results)
    assert len(edt["all"]) == 3 and sorted(edt["mean"]) == ["1", "2", "3"]
    assert np.isfinite(edt["mean"]["2"]["Hausdorff Distance"]) and edt["mean"]["3"]["Hausdorff Distance 95"] > 0
    # labels 2 and 3 go through the histogram: one table visit per case; label 1 (rv_rejection cuts two slices) keeps the per-label route,
    # whose three metrics ask for six directed distance vectors, now from the transform.  Nothing searches over pairs.
    assert "cf_surface_min_dist" not in calls and "cf_surface_border" not in calls
    assert calls.count("cf_label_surface_edt") == 3 * (1 + 6)
    assert calls.count("cf_label_confusion") == 3


def test_pairs_route_still_searches(dev, folders, monkeypatch):
    _, _, calls = run(*folders, monkeypatch=monkeypatch, surface="pairs")
    assert "cf_label_surface_edt" not in calls and calls.count("cf_surface_min_dist") == 3 * 3 * 6


def test_surface_dice_adds_one_key_and_changes_nothing_else(dev, folders, pairs_results):
    from cineflow import metrics as M
    from cineflow.evaluation import SURFACE_DICE
    from cineflow.nifti import read_nifti
    gt, pred = folders
    with_nsd = {route: run(gt, pred, surface=route, surface_dice_threshold=1.0)[0] for route in ("edt", "pairs")}
    for route, res in with_nsd.items():
        stripped = json.loads(json.dumps(res))
        for case in stripped["all"]:
            for c in "123":
                assert 0.0 <= case[c].pop(SURFACE_DICE) <= 1.0, route
        for c in "123":
            stripped["mean"][c].pop(SURFACE_DICE)
        same(stripped, pairs_results)
    assert SURFACE_DICE not in pairs_results["all"][0]["1"] and SURFACE_DICE not in pairs_results["mean"]["1"]
    for i, case in enumerate(with_nsd["edt"]["all"]):
        test, _ = read_nifti(case["test"])
        ref, _ = read_nifti(case["reference"])
        for c, cut in ((1, 2), (2, 0), (3, 0)):
            want = M.normalized_surface_dice((test == c)[cut:], (ref == c)[cut:], 1.0, (2.5, 0.78125, 0.78125), method="pairs")
            assert case[str(c)][SURFACE_DICE] == want == with_nsd["pairs"]["all"][i][str(c)][SURFACE_DICE], (i, c)


def test_edt_route_repeats_byte_for_byte(dev, folders):
    gt, pred = folders
    docs = []
    for _ in range(2):
        res, raw, _ = run(gt, pred, surface="edt", surface_dice_threshold=1.0)
        docs.append(json.dumps(res, sort_keys=True))
    assert docs[0] == docs[1]


def test_command_line_writes_the_same_document(dev, folders, tmp_path):
    from cineflow import evaluation as E
    gt, pred = folders
    api = run(gt, pred, surface="edt", surface_dice_threshold=1.0)[0]
    copy = str(tmp_path / "pred")
    shutil.copytree(pred, copy)
    os.remove(os.path.join(copy, "summary.json"))
    E.main(["-ref", gt, "-pred", copy, "-l", "1", "2", "3", "--surface", "edt", "--surface_dice", "1.0"])
    cli = json.loads(open(os.path.join(copy, "summary.json")).read())["results"]
    for a, b in zip(api["all"], cli["all"]):
        a, b = dict(a), dict(b)
        assert os.path.basename(a.pop("test")) == os.path.basename(b.pop("test"))
        a.pop("reference"), b.pop("reference")
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert json.dumps(api["mean"], sort_keys=True) == json.dumps(cli["mean"], sort_keys=True)
