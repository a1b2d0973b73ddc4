"""Exact comparison of the plain data the planning and preprocessing drivers pickle (plans, properties, fingerprints) with what the
reference wrote: same keys in the same containers, equal ints and strings, arrays equal element for element with the same dtype kind,
floats equal bit for bit (NaN equals NaN)."""
import os

import numpy as np


def relative_paths(obj, root):
    """every string below `root` -> its path relative to root, as tests/golden/make_golden_plan_and_preprocess.py stores them"""
    if isinstance(obj, str):
        return os.path.relpath(obj, root) if obj.startswith(root) else obj
    if isinstance(obj, dict):
        out = type(obj)()
        for k, v in obj.items():
            out[k] = relative_paths(v, root)
        return out
    if isinstance(obj, (list, tuple)):
        return type(obj)(relative_paths(v, root) for v in obj)
    return obj


def _is_float(v):
    return isinstance(v, (float, np.floating))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def assert_same(got, want, where=""):
    if isinstance(want, dict):
        assert isinstance(got, dict), (where, type(got))
        assert set(got.keys()) == set(want.keys()), (where, sorted(map(str, got.keys())), sorted(map(str, want.keys())))
        for k in want:
            assert_same(got[k], want[k], "%s[%r]" % (where, k))
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray), (where, type(got))
        assert got.shape == want.shape and got.dtype.kind == want.dtype.kind, (where, got.shape, got.dtype, want.shape, want.dtype)
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), (where, got, want)
    elif isinstance(want, (list, tuple)):
        # a sequence of numbers may be a list, a tuple or torch.Size-made tuple; the kind of sequence is part of the contract for lists only
        assert isinstance(got, (list, tuple)) and isinstance(got, list) == isinstance(want, list), (where, type(got), type(want))
        assert len(got) == len(want), (where, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "%s[%d]" % (where, i))
    elif isinstance(want, (bool, np.bool_)):
        assert isinstance(got, (bool, np.bool_)) and bool(got) == bool(want), (where, got, want)
    elif _is_int(want):
        assert _is_int(got) and int(got) == int(want), (where, got, want)
    elif _is_float(want):
        assert _is_float(got), (where, type(got))
        assert np.float64(got).tobytes() == np.float64(want).tobytes() or (np.isnan(got) and np.isnan(want)), (where, got, want)
    else:
        assert type(got) is type(want) and got == want, (where, got, want)
