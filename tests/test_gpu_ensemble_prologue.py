"""cf_ensemble_merge and cf_ensemble_pairs (csrc/ensemble.hip) share the host code ahead of their launch; a refusal made there must still
name the entry point that was called.  The library is called directly; every call below is refused on the host, so nothing is launched and
no pointer is dereferenced."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

PTR = 0x1000                                                       # aligned, never dereferenced


def _merge(h, n, crop, full, lo=(0, 0, 0)):
    members = (ctypes.c_void_p * 16)(*([PTR] * 16))
    return h.cf_ensemble_merge(ctypes.cast(members, ctypes.c_void_p), n, 0, 4, *crop, PTR, *full, *lo, None, None, None)


def _pairs(h, n, crop, full, lo=(0, 0, 0)):
    members = (ctypes.c_void_p * 16)(*([PTR] * 16))
    pairs = (ctypes.c_int * 2)(0, 1)
    return h.cf_ensemble_pairs(ctypes.cast(members, ctypes.c_void_p), n, 0, 4, *crop, ctypes.cast(pairs, ctypes.c_void_p), 1, PTR, PTR, *full, *lo,
                               None, PTR, None)


@pytest.mark.parametrize("call,name,too_few", [(_merge, b"cf_ensemble_merge: ", 0), (_pairs, b"cf_ensemble_pairs: ", 1)])
def test_a_refusal_names_the_entry_point_that_was_called(call, name, too_few):
    from cineflow import _lib
    h = _lib.lib()
    rc = call(h, too_few, (1, 2, 3), (1, 2, 3))                     # the entry's own check: its member-count range
    assert rc != 0 and h.cf_last_error().startswith(name + b"n_members = %d is outside" % too_few), (rc, h.cf_last_error())
    rc = call(h, 2, (1, 2, 4), (1, 2, 3))                           # a shared check: X = 4 in Xf = 3
    assert rc != 0 and h.cf_last_error() == name + b"the crop (1, 2, 4) at (0, 0, 0) overhangs the volume (1, 2, 3)", (rc, h.cf_last_error())
