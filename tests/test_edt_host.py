"""The host side of the distance transform and of the evaluator's EDT route, without a GPU: the three entry points are named by the header,
the binding and the built library; the C calls check their arguments before any device call; the Python wrappers refuse CPU tensors, an
unknown method and the scipy arguments that are not built, all before touching the device; the CLI takes --surface and --surface_dice; and
the surface-Dice arithmetic is right on two hand-made distance vectors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cf_edt", "cf_label_surface_edt", "cf_edt_workspace_bytes")


def test_header_binding_and_library_name_the_entry_points():
    from cineflow import _lib
    header = open(os.path.join(ROOT, "include", "cineflow.h")).read()
    binding = open(_lib.__file__).read()
    h = _lib.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in binding, name
        assert hasattr(h, name), name
    assert h.cf_edt_workspace_bytes.restype is ctypes.c_long


def test_workspace_query_and_argument_checks_need_no_gpu():
    from cineflow import _lib
    h = _lib.lib()
    # about 7 bytes per voxel: flags 1 + x offsets 2 + (x, y) offsets 4, 8 bytes per 256 voxels, a 4 KiB header, sections rounded to 256 bytes
    n = 160 * 384 * 384
    size = h.cf_edt_workspace_bytes(160, 384, 384)
    assert 7 * n + n // 32 + 4096 <= size <= 7 * n + n // 32 + 4096 + 5 * 256
    assert h.cf_edt_workspace_bytes(1, 7, 5) >= 4096 + 7 * 35
    # more than 2^31 bytes: the size is a long
    assert h.cf_edt_workspace_bytes(1024, 1024, 1024) > 7 * 2 ** 30
    assert h.cf_edt_workspace_bytes(0, 4, 4) == -1 and h.cf_edt_workspace_bytes(4, 4, 70000) == -1
    a = 4096
    labels = (ctypes.c_int * 2)(1, 2)
    assert h.cf_edt(None, 1, 4, 4, 2, 1.0, 1.0, 1.0, a, a, None) == -1 and b"null pointer" in h.cf_last_error()
    assert h.cf_edt(a, 2, 4, 4, 2, 1.0, 1.0, 1.0, a, a, None) == -1 and b"ndim" in h.cf_last_error()
    assert h.cf_edt(a, 2, 4, 4, 3, 1.0, 0.0, 1.0, a, a, None) == -1 and b"spacing" in h.cf_last_error()
    assert h.cf_edt(a, 2, 4, 4, 3, 1.0, 1.0, 1.0, a + 4, a, None) == -1 and b"aligned" in h.cf_last_error()
    call = h.cf_label_surface_edt
    assert call(a, a, 2, 4, 4, 3, labels, 0, 1.0, 1.0, 1.0, 0, a, a, 64, a, None) == -1 and b"K must be" in h.cf_last_error()
    assert call(a, a, 2, 4, 4, 3, labels, 17, 1.0, 1.0, 1.0, 0, a, a, 64, a, None) == -1
    assert call(a, a, 2, 4, 4, 3, (ctypes.c_int * 2)(1, 256), 2, 1.0, 1.0, 1.0, 0, a, a, 64, a, None) == -1 and b"uint8" in h.cf_last_error()
    assert call(a, a, 2, 4, 4, 3, labels, 2, 1.0, 1.0, 1.0, 0, a, a, 0, a, None) == -1 and b"capacity" in h.cf_last_error()
    assert call(a, a, 2048, 2048, 2048, 3, labels, 2, 1.0, 1.0, 1.0, 0, a, a, 64, a, None) == -1 and b"2^31" in h.cf_last_error()
    assert call(a, None, 2, 4, 4, 3, labels, 2, 1.0, 1.0, 1.0, 0, a, a, 64, a, None) == -1


def test_wrappers_refuse_cpu_tensors_before_any_device_work():
    from cineflow import metrics as M
    m = torch.zeros(3, 4, 5, dtype=torch.uint8)
    with pytest.raises(TypeError, match="CUDA/HIP tensor"):
        M.distance_transform_edt(m)
    with pytest.raises(TypeError, match="CUDA/HIP tensor"):
        M.surface_distances(m, m, method="edt")
    with pytest.raises(TypeError, match="CUDA/HIP tensor"):
        M.label_surface_edt_table(m, m, [1])
    with pytest.raises(TypeError, match="CUDA/HIP tensor"):
        M.normalized_surface_dice(m, m, 1.0)


def test_bad_method_and_unbuilt_scipy_arguments():
    from cineflow import metrics as M
    from cineflow.evaluation import Evaluator
    m = np.zeros((3, 4, 5), np.uint8)
    with pytest.raises(ValueError, match="method"):
        M.surface_distances(m, m, method="brute")
    with pytest.raises(ValueError, match="surface"):
        Evaluator(labels=[1]).evaluate(m, m, surface="brute")
    for kw, name in (({"return_indices": True}, "return_indices"), ({"return_distances": False}, "return_distances"),
                     ({"distances": np.zeros((3, 4, 5))}, "distances"), ({"indices": np.zeros((3, 3, 4, 5), np.int32)}, "indices")):
        with pytest.raises(NotImplementedError, match=name):
            M.distance_transform_edt(m, **kw)
    with pytest.raises(ValueError, match="labels"):
        M.label_surface_edt_table(m, m, list(range(17)))


def test_parser_accepts_surface_and_surface_dice():
    from cineflow import evaluation as E
    p = E.build_parser()
    a = p.parse_args(["-ref", "r", "-pred", "p", "-l", "1", "2", "3"])
    assert (a.surface, a.surface_dice) == ("auto", None)
    a = p.parse_args(["-ref", "r", "-pred", "p", "-l", "1", "--surface", "edt", "--surface_dice", "1.5"])
    assert (a.surface, a.surface_dice) == ("edt", 1.5)
    assert p.parse_args(["-ref", "r", "-pred", "p", "-l", "1", "--surface", "pairs"]).surface == "pairs"
    with pytest.raises(SystemExit):
        p.parse_args(["-ref", "r", "-pred", "p", "-l", "1", "--surface", "brute"])


def test_main_hands_the_route_and_the_threshold_to_evaluate_folder(monkeypatch):
    from cineflow import evaluation as E
    seen = []
    monkeypatch.setattr(E, "evaluate_folder", lambda *a, **k: seen.append((a, k)))
    E.main(["-ref", "r", "-pred", "p", "-l", "1", "2"])
    E.main(["-ref", "r", "-pred", "p", "-l", "1", "--surface", "edt", "--surface_dice", "2"])
    assert seen == [(("r", "p", [1, 2]), {"surface": "auto"}), (("r", "p", [1]), {"surface": "edt", "surface_dice_threshold": 2.0})]


def test_surface_dice_arithmetic_on_hand_made_distances():
    from cineflow.metrics import surface_dice_from_distances
    a_to_b = np.array([0.0, 0.5, 1.0, 2.0])          # 3 of 4 within 1.0 (<= counts the value AT the threshold)
    b_to_a = np.array([1.0, 1.5, 3.0, 0.25, 4.0])    # 2 of 5 within
    want = (0.75 + 0.4) / (0.75 + 0.4 + 0.25 + 0.6 + 1e-8)
    assert surface_dice_from_distances(a_to_b, b_to_a, 1.0) == want
    assert surface_dice_from_distances(b_to_a, a_to_b, 1.0) == want            # symmetric
    assert surface_dice_from_distances(a_to_b, b_to_a, 0.0) == (0.25 + 0.0) / (0.25 + 0.0 + 0.75 + 1.0 + 1e-8)
    assert surface_dice_from_distances(a_to_b, b_to_a, 4.0) == 2.0 / (2.0 + 1e-8)
    assert surface_dice_from_distances(a_to_b, b_to_a, 0.999) == (0.5 + 0.2) / (0.5 + 0.2 + 0.5 + 0.8 + 1e-8)
