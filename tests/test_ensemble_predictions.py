"""cineflow.ensemble_predictions without a GPU: case discovery, the refusals that come before any device work, the CLI parser, override=False,
and the host-side argument validation of cf_ensemble_merge (which launches nothing when it refuses)."""
import ctypes
import os
import pickle

import numpy as np
import pytest


def _props(shape, full=None, lo=(0, 0, 0), **extra):
    full = tuple(shape) if full is None else tuple(full)
    p = {"size_after_cropping": tuple(shape), "original_size_of_raw_data": np.array(full),
         "crop_bbox": [[a, a + n] for a, n in zip(lo, shape)], "itk_spacing": (1.5, 1.5, 8.0), "itk_origin": (0.0, 0.0, 0.0),
         "itk_direction": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)}
    p.update(extra)
    return p


def _write_case(folder, case, softmax=None, props=None, npz=True, pkl=True):
    path = os.path.join(str(folder), case)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    softmax = np.full((2, 1, 2, 3), 0.5, np.float16) if softmax is None else softmax
    if npz:
        np.savez_compressed(path + ".npz", softmax=softmax)
    if pkl:
        with open(path + ".pkl", "wb") as f:
            pickle.dump(_props(softmax.shape[1:]) if props is None else props, f)


def test_find_cases_flat_nested_and_mixed(tmp_path):
    from cineflow import ensemble_predictions as E
    flat, nested, mixed = tmp_path / "flat", tmp_path / "nested", tmp_path / "mixed"
    for c in ("b_case", "a_case"):
        _write_case(flat, c)
    for c in ("p2/p2_f00", "p1/p1_f01", "p1/p1_f00"):
        _write_case(nested, c)
    _write_case(mixed, "a_case")
    _write_case(mixed, "p1/p1_f00")
    _write_case(mixed, "p1/deeper/too_deep")                       # two levels down: not a case
    (mixed / "notes.txt").write_text("x")
    (mixed / "p1" / "p1_f00.nii.gz").write_text("x")
    assert E.find_cases([str(flat)]) == ["a_case", "b_case"]
    assert E.find_cases([str(nested)]) == [os.path.join("p1", "p1_f00"), os.path.join("p1", "p1_f01"), os.path.join("p2", "p2_f00")]
    assert E.find_cases([str(mixed)]) == ["a_case", os.path.join("p1", "p1_f00")]
    assert E.find_cases([str(flat), str(mixed)]) == ["a_case", "b_case", os.path.join("p1", "p1_f00")]       # the union, sorted


@pytest.mark.parametrize("missing,message", [("npz", "Not all patient npz are available in all folders"),
                                             ("pkl", "Not all patient pkl are available in all folders")])
def test_a_folder_that_lacks_a_file_is_refused_before_anything_is_read(tmp_path, monkeypatch, missing, message):
    from cineflow import ensemble_predictions as E
    a, b = tmp_path / "a", tmp_path / "b"
    for c in ("p1/c0", "p1/c1"):
        _write_case(a, c)
    _write_case(b, "p1/c0")
    _write_case(b, "p1/c1", npz=missing != "npz", pkl=missing != "pkl")

    def no_read(*_a, **_k):
        raise RuntimeError("a file was read")
    monkeypatch.setattr(E, "_load_softmax", no_read)
    monkeypatch.setattr(E, "load_plain_pickle", no_read)
    with pytest.raises(AssertionError) as e:
        E.merge([str(a), str(b)], str(tmp_path / "out"), 2)
    assert str(e.value) == message


def test_regions_class_orders_must_agree(tmp_path):
    from cineflow import ensemble_predictions as E
    a, b = tmp_path / "a", tmp_path / "b"
    sm = np.full((3, 1, 2, 3), 0.25, np.float16)
    _write_case(a, "c0", sm, _props(sm.shape[1:], regions_class_order=(3, 1, 2)))
    _write_case(b, "c0", sm, _props(sm.shape[1:], regions_class_order=(1, 2, 3)))
    with pytest.raises(AssertionError, match="the regions_class_orders of all files must be the same"):
        E.merge([str(a), str(b)], str(tmp_path / "out"), 1)
    files = [[str(f / "c0") + e for f in (a, b)] for e in (".npz", ".pkl")]
    with pytest.raises(AssertionError, match="the regions_class_orders of all files must be the same"):
        E.merge_files(files[0], files[1], str(tmp_path / "out" / "c0.nii.gz"), True, False)


def test_shape_refusals_name_the_case_and_the_shapes(tmp_path):
    from cineflow import ensemble_predictions as E
    a, b = tmp_path / "a", tmp_path / "b"
    _write_case(a, "c0", np.full((2, 1, 2, 3), 0.5, np.float16))
    _write_case(b, "c0", np.full((2, 1, 2, 4), 0.5, np.float16))                              # another shape
    _write_case(a, "c1", np.full((2, 1, 2, 3), 0.5, np.float16))
    _write_case(b, "c1", np.full((3, 1, 2, 3), 0.5, np.float16))                              # another class count
    _write_case(a, "c2", np.full((2, 1, 2, 3), 0.5, np.float16), _props((1, 4, 6)))           # not the size after cropping
    _write_case(b, "c2", np.full((2, 1, 2, 3), 0.5, np.float16), _props((1, 4, 6)))
    _write_case(a, "c3", np.full((2, 1, 2, 3), 0.5, np.float16), _props((1, 2, 3), (1, 2, 4), (0, 0, 2)))   # overhangs x
    _write_case(b, "c3", np.full((2, 1, 2, 3), 0.5, np.float16), _props((1, 2, 3), (1, 2, 4), (0, 0, 2)))
    _write_case(a, "c4", np.full((2, 1, 2, 3), 0.5, np.float16))
    _write_case(b, "c4", np.full((2, 1, 2, 3), 0.5, np.float32))                              # another dtype
    out = str(tmp_path / "out" / "c.nii.gz")

    def one(case):
        files = [[str(f / case) + e for f in (a, b)] for e in (".npz", ".pkl")]
        return E.merge_files(files[0], files[1], out, True, False)
    with pytest.raises(ValueError, match=r"c0\.npz.*\(2, 1, 2, 3\).*\(2, 1, 2, 4\)"):
        one("c0")
    with pytest.raises(ValueError, match=r"c1\.npz.*\(2, 1, 2, 3\).*\(3, 1, 2, 3\)"):
        one("c1")
    with pytest.raises(ValueError, match=r"c2\.npz.*\(1, 2, 3\).*size_after_cropping is \(1, 4, 6\)"):
        one("c2")
    with pytest.raises(ValueError, match=r"c3\.npz.*overhangs"):
        one("c3")
    with pytest.raises(ValueError, match=r"c4\.npz.*float16.*float32"):
        one("c4")
    assert not os.path.exists(out)


def test_property_files_go_through_the_restricted_unpickler(tmp_path):
    import subprocess
    from cineflow import ensemble_predictions as E
    a = tmp_path / "a"
    _write_case(a, "c0", pkl=False)
    with open(str(a / "c0.pkl"), "wb") as f:
        pickle.dump({"size_after_cropping": (1, 2, 3), "fn": subprocess.run}, f)
    with pytest.raises(pickle.UnpicklingError, match="refusing to load global"):
        E.merge_files([str(a / "c0.npz")], [str(a / "c0.pkl")], str(tmp_path / "c0.nii.gz"), True, False)


def test_cli_flags_and_defaults():
    from cineflow import ensemble_predictions as E
    p = E.build_parser()
    a = p.parse_args(["-f", "x", "y", "z", "-o", "out"])
    assert a.folders == ["x", "y", "z"] and a.output_folder == "out"
    assert a.threads == 2 and a.postprocessing_file is None and a.npz is False
    a = p.parse_args(["--folders", "x", "--output_folder", "o", "--threads", "5", "--postprocessing_file", "pp.json", "--npz"])
    assert a.folders == ["x"] and a.output_folder == "o" and a.threads == 5 and a.postprocessing_file == "pp.json" and a.npz is True
    a = p.parse_args(["-f", "x", "-o", "o", "-t", "3", "-pp", "q.json"])
    assert a.threads == 3 and a.postprocessing_file == "q.json"
    for argv in (["-o", "out"], ["-f", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_public_names_and_argument_lists_are_the_references():
    import inspect
    from cineflow import ensemble_predictions as E
    assert list(inspect.signature(E.merge_files).parameters) == ["files", "properties_files", "out_file", "override", "store_npz"]
    sig = inspect.signature(E.merge)
    assert list(sig.parameters) == ["folders", "output_folder", "threads", "override", "postprocessing_file", "store_npz"]
    assert sig.parameters["override"].default is True and sig.parameters["postprocessing_file"].default is None
    assert sig.parameters["store_npz"].default is False
    assert callable(E.main)


def test_override_false_leaves_existing_outputs_alone(tmp_path, monkeypatch):
    from cineflow import ensemble_predictions as E
    a, b, out = tmp_path / "a", tmp_path / "b", tmp_path / "out"
    for f in (a, b):
        _write_case(f, "p1/c0")
        _write_case(f, "c1")
    targets = [out / "p1" / "c0.nii.gz", out / "c1.nii.gz"]
    (out / "p1").mkdir(parents=True)
    for t in targets:
        t.write_bytes(b"already there")
        os.utime(str(t), ns=(1_000_000_000, 1_000_000_000))

    def no_read(*_a, **_k):
        raise RuntimeError("a member was read")
    monkeypatch.setattr(E, "_load_softmax", no_read)
    monkeypatch.setattr(E, "load_plain_pickle", no_read)
    E.merge([str(a), str(b)], str(out), 2, override=False)
    E.merge_files([str(a / "c1.npz"), str(b / "c1.npz")], [str(a / "c1.pkl"), str(b / "c1.pkl")], str(targets[1]), False, False)
    for t in targets:
        assert os.stat(str(t)).st_mtime_ns == 1_000_000_000 and t.read_bytes() == b"already there"


def test_ops_refuses_cpu_tensors_and_names_the_offending_member():
    import torch
    from cineflow import ops
    with pytest.raises(TypeError, match="member 0 must be a CUDA/HIP tensor"):
        ops.ensemble_merge([torch.zeros(2, 1, 2, 3, dtype=torch.float16)])
    with pytest.raises(ValueError, match="0 members"):
        ops.ensemble_merge([])


# ------------------------------------------------------------------------------------------------ cf_ensemble_merge: host-side validation
def _call(h, n=2, dtype=0, K=4, crop=(5, 13, 17), full=(7, 16, 24), lo=(1, 2, 3), members=True, seg=1, order=None):
    ptrs = (ctypes.c_void_p * 17)(*([0x1000] * 17))                 # never dereferenced on the device: every call below is refused on the host
    return h.cf_ensemble_merge(ctypes.cast(ptrs, ctypes.c_void_p) if members else None, n, dtype, K, *crop, seg, *full, *lo, None, order, None)


@pytest.mark.parametrize("kwargs,text", [(dict(n=0), b"n_members = 0 is outside 1..16"),
                                         (dict(n=17), b"n_members = 17 is outside 1..16"),
                                         (dict(lo=(1, 2, 8)), b"overhangs the volume"),           # 8 + 17 > 24
                                         (dict(lo=(3, 2, 3)), b"overhangs the volume"),           # 3 + 5 > 7
                                         (dict(lo=(1, 4, 3)), b"overhangs the volume"),           # 4 + 13 > 16
                                         (dict(lo=(-1, 2, 3)), b"overhangs the volume"),
                                         (dict(dtype=2), b"dtype = 2"),
                                         (dict(dtype=-1), b"dtype = -1"),
                                         (dict(K=0), b"K = 0 is outside 1..255"),
                                         (dict(K=256), b"K = 256 is outside 1..255"),
                                         (dict(crop=(5, 0, 17)), b"bad shape"),
                                         (dict(members=False), b"null pointer"),
                                         (dict(seg=None), b"null pointer")])
def test_cf_ensemble_merge_validates_on_the_host(kwargs, text):
    from cineflow import _lib
    h = _lib.lib()
    rc = _call(h, **kwargs)
    assert rc < 0 and text in h.cf_last_error(), (rc, h.cf_last_error())


def test_cf_ensemble_merge_refuses_a_null_member():
    from cineflow import _lib
    h = _lib.lib()
    ptrs = (ctypes.c_void_p * 2)(0x1000, None)
    rc = h.cf_ensemble_merge(ctypes.cast(ptrs, ctypes.c_void_p), 2, 0, 4, 5, 13, 17, 1, 7, 16, 24, 1, 2, 3, None, None, None)
    assert rc < 0 and b"member 1 is a null pointer" in h.cf_last_error()
