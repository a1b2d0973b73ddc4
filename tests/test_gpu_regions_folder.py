"""A region-based folder through the file-level API: import of the 3-D fixture (tests/golden/ref_model_regions), predict_from_folder with
save_npz, cineflow.ensemble_predictions on the folder it wrote, and the region-based evaluation.

Bars: tests/_region_refs.py -- label files equal the fixture's labels outside the voxels where a reference probability lies within
bar_p = 2.7e-5 of 0.5 (at most 0.5 % of the voxels); the .npz holds the fp16 rounding of probabilities within bar_p of the fixture's, so it
is held to bar_p + 2^-11 |p| (fp16's unit roundoff) -- except the values export.probabilities_as_stored rounds up instead of to nearest
(p in (0.5, 0.5 + 2^-12], stored as 0.5 + 2^-11 so that `stored > 0.5` where `p > 0.5`): each of those must be exactly that fp16 value over a
reference probability that lies in that interval widened by bar_p.  The ensemble of the folder and its copy must then write the folder's own
label file, voxel for voxel.  summary.csv is compared character for character with a numpy restatement.

The case file holds the fixture's `raw` volume; the plans' preprocessing (z-score per modality, the files carry the stage's spacing, no
voxel is zero so nothing is cropped) gives the fixture's `volume` up to fp32 rounding.

Measured on the MI355X: the label file differs from the fixture's labels in 0 of 5376 voxels (ambiguous share 0.093 %); the .npz lies
within fp16 storage of the fixture's probabilities (excess -9.5e-7 against the 2.7e-5 bar; the rule rounds 44 values up on the fixture's own probabilities); the ensemble of two copies
differs from the prediction's label file in 0 voxels (21 with plain round-to-nearest storage); summary.csv equal character for character."""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import _region_refs as RR

pytestmark = pytest.mark.gpu
ORDER = (1, 2, 3)
PAT, CASE = "patient001", "patient001_frame01"


@pytest.fixture(scope="module")
def predicted(tmp_path_factory):
    """(output folder of predict_from_folder(save_npz=True) on the fixture's case, its return value)"""
    from cineflow import predict as P
    from cineflow import reference_models as R
    from cineflow.nifti import write_nifti
    base = tmp_path_factory.mktemp("regions_folder")
    model = str(base / "model")
    R.import_reference_model_folder(RR.folder("3d", str(base / "ref")), None, model)
    raw = RR.expected("3d")["raw"].numpy()
    (base / "in" / PAT).mkdir(parents=True)
    for m in range(raw.shape[0]):
        write_nifti(str(base / "in" / PAT / ("%s_%04d.nii.gz" % (CASE, m))), raw[m], (1.5, 1.5, 10.0), (0, 0, 0))      # the stage's own spacing
    out = str(base / "out")
    res = P.predict_from_folder(model, str(base / "in"), out, [0], True, 1, 1, None, 0, 1, True)
    return out, res


def test_predict_from_folder_writes_region_labels(dev, predicted):
    from cineflow.nifti import read_nifti
    print()
    out, res = predicted
    exp = RR.expected("3d")
    ref_p, ref_s = exp["probs"].numpy(), exp["seg"].numpy()
    assert res == {PAT: [os.path.join(out, PAT, CASE + ".nii.gz")]}
    assert sorted(os.listdir(os.path.join(out, PAT))) == [CASE + e for e in (".nii.gz", ".npz", ".pkl")]
    seg, props = read_nifti(os.path.join(out, PAT, CASE + ".nii.gz"))
    assert seg.dtype == np.uint8 and seg.shape == ref_s.shape and np.allclose(props["itk_spacing"], (1.5, 1.5, 10.0))
    amb = RR.ambiguous(ref_p)
    differ, differ_clear = int((seg != ref_s).sum()), int(((seg != ref_s) & ~amb).sum())
    sm = np.load(os.path.join(out, PAT, CASE + ".npz"))["softmax"]
    assert sm.dtype == np.float16 and sm.shape == ref_p.shape
    above = np.nextafter(np.float16(0.5), np.float16(1))
    up = (sm == above) & (ref_p <= 0.5 + 2.0 ** -12 + RR.BAR_P)                 # candidates for the round-up rule: checked exactly, below
    assert bool((ref_p[up] > 0.5 - RR.BAR_P).all())
    excess = float((np.abs(sm.astype(np.float64) - ref_p) - 2.0 ** -11 * np.abs(ref_p))[~up].max())
    print("  label file: %d voxels differ from the fixture's, %d of them unambiguous (ambiguous share %.4f %%); .npz beyond fp16 storage: %.3e "
          "(bar %.2e), %d values rounded up to %.8f" % (differ, differ_clear, 100 * amb.mean(), excess, RR.BAR_P, int(up.sum()), float(above)))
    assert amb.mean() <= RR.AMBIGUOUS_CAP and differ_clear == 0
    assert excess <= RR.BAR_P
    assert np.array_equal(RR.region_labels(sm, ORDER), seg)                     # the stored member says what its label file says
    with open(os.path.join(out, PAT, CASE + ".pkl"), "rb") as f:
        pkl = pickle.load(f)
    assert list(pkl["regions_class_order"]) == list(ORDER)


def test_ensemble_of_two_copies_is_the_region_rule_on_the_stored_probabilities(dev, predicted, tmp_path):
    """the -z folder is a valid member with no further flag: the members' .pkl carries the order, and the merged labels are the region
    rule on the mean of the stored (fp16) probabilities -- which for two copies is the stored value itself"""
    from cineflow import ensemble_predictions as E
    from cineflow.nifti import read_nifti
    out, _ = predicted
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    shutil.copytree(os.path.join(out, PAT), a)
    shutil.copytree(os.path.join(out, PAT), b)
    E.merge([a, b], str(tmp_path / "merged"), 1)
    merged, _ = read_nifti(str(tmp_path / "merged" / (CASE + ".nii.gz")))
    sm = np.load(os.path.join(a, CASE + ".npz"))["softmax"]
    assert np.array_equal(merged, RR.region_labels(sm, ORDER))
    assert set(np.unique(merged)) <= {0, 1, 2, 3} and len(np.unique(merged)) >= 3


def test_ensemble_of_two_copies_writes_the_same_label_file(dev, predicted, tmp_path):
    """The ensemble of two copies of the -z folder writes the label file the prediction wrote, voxel for voxel.

    The prediction's labels are the region rule on the fp32 probabilities (segmentation_export.py:145-150), the ensemble's on the fp16
    values the .npz stores.  With plain round-to-nearest storage a probability in (0.5, 0.5 + 2^-12] is stored as 0.5 and is no longer
    `> 0.5`: 21 of the 5376 voxels of this case changed their label that way (measured, and the same count on the fixture's own
    probabilities without the device).  export.probabilities_as_stored rounds those values up instead, so the two files are equal."""
    from cineflow import ensemble_predictions as E
    from cineflow.nifti import read_nifti
    print()
    out, _ = predicted
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    shutil.copytree(os.path.join(out, PAT), a)
    shutil.copytree(os.path.join(out, PAT), b)
    E.merge([a, b], str(tmp_path / "merged"), 1)
    merged, _ = read_nifti(str(tmp_path / "merged" / (CASE + ".nii.gz")))
    seg, _ = read_nifti(os.path.join(out, PAT, CASE + ".nii.gz"))
    print("  ensemble of two copies vs the prediction's label file: %d of %d voxels differ" % (int((merged != seg).sum()), seg.size))
    assert np.array_equal(merged, seg)


# ------------------------------------------------------------------------------------------------ region-based evaluation
def _dice(pred, gt, labels):
    p, g = np.isin(pred, labels), np.isin(gt, labels)
    if not p.any() and not g.any():
        return np.nan
    return 2.0 * np.logical_and(p, g).sum() / float(p.sum() + g.sum())


def _summary(cases, regions):
    """numpy restatement of region_based_evaluation.py's summary.csv"""
    names = list(regions)
    lines = ["casename" + "".join(",%s" % r for r in names)]
    table = []
    for name, pred, gt in cases:
        table.append([_dice(pred, gt, list(regions[r])) for r in names])
        lines.append(name + "".join(",%02.4f" % v for v in table[-1]))
    t = np.array(table, dtype=np.float64)
    one = np.where(np.isnan(t), 1.0, t)
    for title, values in (("mean", np.nanmean(t, 0)), ("median", np.nanmedian(t, 0)), ("mean (nan is 1)", one.mean(0)),
                          ("median (nan is 1)", np.median(one, 0))):
        lines.append(title + "".join(",%02.4f" % v for v in values))
    return "\n".join(lines) + "\n"


def test_evaluate_regions_writes_the_reference_summary(dev, tmp_path, capsys):
    from cineflow import evaluation as EV
    from cineflow.nifti import write_nifti
    assert EV.get_brats_regions() == {"whole tumor": (1, 2, 3), "tumor core": (2, 3), "enhancing tumor": (3,)}
    assert list(EV.get_brats_regions()) == ["whole tumor", "tumor core", "enhancing tumor"]
    assert EV.get_KiTS_regions() == {"kidney incl tumor": (1, 2), "tumor": (2,)}
    m = EV.create_region_from_mask(np.array([[0, 1], [2, 3]]), (2, 3))
    assert m.dtype == np.uint8 and np.array_equal(m, [[0, 0], [1, 1]])
    rng = np.random.RandomState(17)
    gt_dir, pred_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pred_dir.mkdir()
    cases = []
    for i in range(4):
        gt = rng.randint(0, 4, size=(5, 12, 10)).astype(np.uint8)
        pred = np.where(rng.rand(5, 12, 10) < 0.8, gt, rng.randint(0, 4, size=(5, 12, 10))).astype(np.uint8)
        if i == 1:                                         # enhancing tumour empty in both: NaN, and the "nan is 1" rows differ
            gt[gt == 3] = 2
            pred[pred == 3] = 1
        if i == 2:                                         # empty in the prediction alone: a Dice of 0, not NaN
            pred[pred == 3] = 0
        name = "case_%02d" % i
        write_nifti(str(gt_dir / (name + ".nii.gz")), gt, (1.0, 1.0, 5.0), (0, 0, 0))
        write_nifti(str(pred_dir / (name + ".nii.gz")), pred, (1.0, 1.0, 5.0), (0, 0, 0))
        cases.append((name, pred, gt))
    write_nifti(str(gt_dir / "case_99.nii.gz"), cases[0][2], (1.0, 1.0, 5.0), (0, 0, 0))          # ground truth without a prediction: a warning
    regions = EV.get_brats_regions()
    scores = EV.evaluate_regions(str(pred_dir), str(gt_dir), regions, processes=2)
    assert "WARNING! Some files in folder_gt were not predicted" in capsys.readouterr().out
    want = _summary(cases, regions)
    with open(str(pred_dir / "summary.csv")) as f:
        got = f.read()
    assert got == want, "\n" + got + "\n" + want
    assert "nan" in got.splitlines()[2] and got.splitlines()[5] != got.splitlines()[7].replace("mean (nan is 1)", "mean")
    assert np.isnan(scores["enhancing tumor"][1]) and scores["enhancing tumor"][2] == 0.0
    assert EV.evaluate_case(str(pred_dir / "case_00.nii.gz"), str(gt_dir / "case_00.nii.gz"), list(regions.values())) == \
        [scores[r][0] for r in regions]
    # the command line, with a JSON region set
    os.remove(str(pred_dir / "summary.csv"))
    EV.main(["--regions", '{"kidney incl tumor": [1, 2], "tumor": [2]}', "-ref", str(gt_dir), "-pred", str(pred_dir)])
    with open(str(pred_dir / "summary.csv")) as f:
        assert f.read() == _summary(cases, EV.get_KiTS_regions())
    # a prediction without ground truth is refused
    write_nifti(str(pred_dir / "case_77.nii.gz"), cases[0][1], (1.0, 1.0, 5.0), (0, 0, 0))
    with pytest.raises(AssertionError, match="have not ground truth"):
        EV.evaluate_regions(str(pred_dir), str(gt_dir), regions)
