"""compress="device" end to end: the containers cineflow/deflate.py writes around the device's streams are read by numpy, zipfile and the
NIfTI reader to the very arrays that went in, the same arrays give the same file bytes, and the two commands that take --compress write
folders whose CONTENT equals the default route's file for file (bytes and sizes of the compressed files differ, nothing inside does)."""
import os
import pickle
import shutil
import zipfile

import numpy as np
import pytest
import torch

from _plan_compare import assert_same, relative_paths
from test_gpu_plan_and_preprocess import SEEDED, TASK
from test_gpu_validate import FOLDS, PLANS_PKL, STAGES, VAL, plans_of, same_json, same_value, save_seeded_model

pytestmark = pytest.mark.gpu


def _arrays():
    rs = np.random.RandomState(12)
    lab = (rs.rand(5, 60, 44) * 3).astype(np.uint8)
    return {"data": rs.randn(3, 5, 60, 44).astype(np.float32), "softmax": rs.rand(3, 5, 60, 44).astype(np.float16), "seg": lab,
            "locations": rs.randint(0, 60, (70, 3)).astype(np.int64), "empty": np.zeros((0, 7), np.float32), "mask": lab > 1}


def test_savez_compressed_on_device_tensors(tmp_path):
    from cineflow import deflate
    arrays = _arrays()
    tensors = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    tensors["locations"] = arrays["locations"]                       # a numpy value is uploaded
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b")
    deflate.savez_compressed(a, **tensors)
    deflate.savez_compressed(b, **tensors)                           # numpy's rule: .npz is appended
    assert open(a, "rb").read() == open(b + ".npz", "rb").read()
    with np.load(a) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, v in arrays.items():
            assert z[k].dtype == v.dtype and z[k].shape == v.shape and z[k].tobytes() == v.tobytes(), k
    with zipfile.ZipFile(a) as z:
        assert z.testzip() is None and all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
    np.savez_compressed(str(tmp_path / "ref.npz"), **arrays)
    print("npz bytes: device %d, numpy (zlib level 6) %d" % (os.path.getsize(a), os.path.getsize(str(tmp_path / "ref.npz"))))
    # a view: the bytes of the C-order array it stands for
    view = tensors["data"][:, 1:, ::2]
    deflate.savez_compressed(str(tmp_path / "view.npz"), data=view)
    assert np.array_equal(np.load(str(tmp_path / "view.npz"))["data"], arrays["data"][:, 1:, ::2])


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_write_nifti_on_the_device(tmp_path, dtype):
    from cineflow.nifti import read_nifti, write_nifti
    vol = (np.random.RandomState(1).rand(6, 50, 37) * 4).astype(dtype)
    geo = ((0.8, 0.9, 3.0), (5.0, -7.0, 11.0), (0, 1, 0, -1, 0, 0, 0, 0, 1))
    ref, dev_t, dev_n, twice = (str(tmp_path / n) for n in ("ref.nii.gz", "dev_t.nii.gz", "dev_n.nii.gz", "twice.nii.gz"))
    write_nifti(ref, vol, *geo)
    write_nifti(dev_t, torch.from_numpy(vol).cuda(), *geo, compress="device")
    write_nifti(dev_n, vol, *geo, compress="device")
    write_nifti(twice, torch.from_numpy(vol).cuda(), *geo, compress="device")
    want, want_props = read_nifti(ref)
    for path in (dev_t, dev_n):
        got, props = read_nifti(path)
        assert got.dtype == vol.dtype and np.array_equal(got, vol) and np.array_equal(got, want) and props == want_props
    assert open(dev_t, "rb").read() == open(twice, "rb").read() == open(dev_n, "rb").read()
    plain = str(tmp_path / "plain.nii")                              # no .gz: nothing to compress, the same file as the default route's
    write_nifti(plain, torch.from_numpy(vol).cuda(), *geo, compress="device")
    write_nifti(str(tmp_path / "plain_ref.nii"), vol, *geo)
    assert open(plain, "rb").read() == open(str(tmp_path / "plain_ref.nii"), "rb").read()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def _load(path):
    from cineflow.safe_pickle import load_plain_pickle
    return load_plain_pickle(path)


def _same_npz(a, b):
    with np.load(a) as x, np.load(b) as y:
        assert sorted(x.files) == sorted(y.files), a
        for k in x.files:
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (a, k)
    with zipfile.ZipFile(a) as z:
        assert z.testzip() is None, a


def test_plan_and_preprocess_folders_equal_the_default_route(dev, tmp_path):
    from cineflow import plan_and_preprocess as PP
    out = {}
    for compress in ("zlib", "device"):              # the same layout under two roots: the pickles name files, compared relative to their root
        root = str(tmp_path / compress)
        raw, cropped, pre = (os.path.join(root, d, TASK) for d in ("nnUNet_raw_data", "nnUNet_cropped_data", "nnUNet_preprocessed"))
        shutil.copytree(os.path.join(SEEDED, "raw"), raw)
        assert PP.main(["--raw", raw, "--cropped", cropped, "--preprocessed", pre, "-tf", "8", "--compress", compress]) == 0
        out[compress] = (cropped, pre)
    sizes = {}
    for i in (0, 1):
        a, b = out["zlib"][i], out["device"][i]
        assert _tree(a) == _tree(b)
        for rel in _tree(a):
            fa, fb = os.path.join(a, rel), os.path.join(b, rel)
            if rel.endswith(".npz"):
                _same_npz(fb, fa)
                sizes[i] = tuple(x + y for x, y in zip(sizes.get(i, (0, 0)), (os.path.getsize(fa), os.path.getsize(fb))))
            elif rel.endswith(".pkl"):
                assert_same(relative_paths(_load(fb), str(tmp_path / "device")), relative_paths(_load(fa), str(tmp_path / "zlib")), rel)   # case properties, fingerprint, plans
            else:
                assert open(fa, "rb").read() == open(fb, "rb").read(), rel    # label files, dataset.json: copies
    assert sizes[0][0] and sizes[1][0]
    print("npz bytes zlib / device: cropped %d / %d, stage folders %d / %d" % (sizes[0] + sizes[1]))


def test_validate_folders_equal_the_default_route(dev, tmp_path):
    """the 3-D network, whose softmax is equal bit for bit from run to run (test_gpu_validate.py), fold 1 (two cases), with the next
    stage's label files"""
    from cineflow import validate as V
    from cineflow.nifti import read_nifti
    pre = str(tmp_path / "preprocessed")
    shutil.copytree(os.path.join(SEEDED, "preprocessed"), pre)
    cases = sorted(c for f in FOLDS for c in f)
    with open(os.path.join(pre, "splits_final.pkl"), "wb") as f:
        pickle.dump([{"train": np.array(sorted(set(cases) - set(val))), "val": np.array(val)} for val in FOLDS], f)
    gt = os.path.join(SEEDED, "raw", "labelsTr")
    stage = os.path.join(pre, STAGES["3d"])
    model = save_seeded_model(str(tmp_path / "model"), plans_of("3d"), dev, (30, 40))
    exp = {}
    for compress in ("zlib", "device"):
        exp[compress] = str(tmp_path / compress / "exp")             # (summary.json names the experiment folder's last part)
        V.main(["-m", model, "--data", stage, "-gt", gt, "-o", exp[compress], "--plans", os.path.join(pre, PLANS_PKL["3d"]), "-t", TASK, "-f", "1",
                "--next_stage", stage, "--compress", compress])
    a, b = exp["zlib"], exp["device"]
    assert _tree(a) == _tree(b)
    raw_a = os.path.join(a, "fold_1", VAL)
    assert sorted(f for f in os.listdir(raw_a) if f.endswith(".npz")) == [c + ".npz" for c in FOLDS[1]]
    for rel in _tree(a):
        fa, fb = os.path.join(a, rel), os.path.join(b, rel)
        if rel.endswith(".npz"):
            _same_npz(fb, fa)
        elif rel.endswith(".nii.gz"):
            (va, pa), (vb, pb) = read_nifti(fa), read_nifti(fb)
            assert va.dtype == vb.dtype and np.array_equal(va, vb) and pa == pb, rel
        elif rel.endswith(".json"):
            import json
            da, db = json.load(open(fa)), json.load(open(fb))
            for d in (da, db):                                        # the documents name their own experiment folder and the clock
                d.pop("timestamp", None)
                d.pop("id", None)
            assert same_json(_strip(da, a), _strip(db, b)), rel
        elif rel.endswith(".pkl"):
            assert same_value(_load(fa), _load(fb)), rel
    assert len(np.unique(read_nifti(os.path.join(b, "fold_1", VAL, FOLDS[1][0] + ".nii.gz"))[0])) > 1


def _strip(doc, root):
    """a JSON document with every occurrence of its experiment folder's path cut out of its strings"""
    if isinstance(doc, dict):
        return {k: _strip(v, root) for k, v in doc.items()}
    if isinstance(doc, list):
        return [_strip(v, root) for v in doc]
    if isinstance(doc, str):
        return doc.replace(root, "")
    return doc
