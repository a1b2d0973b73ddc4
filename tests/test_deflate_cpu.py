"""CPU tests (no GPU) of the device-DEFLATE route: the CRC arithmetic and the zip / gzip containers of cineflow/deflate.py with a host
stand-in for the kernel (zlib raw deflate per chunk, each ended with a sync flush: the shape of stream csrc/deflate.hip writes), the host
side of cf_deflate / cf_crc32 (argument checks before any launch, the bound), and the kernel's own text -- csrc/deflate_core.h -- run on
one host thread against zlib by tools/deflate_hostcheck.cpp."""
import ctypes
import gzip
import io
import os
import shutil
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_bytes(n, seed=0):
    return np.random.RandomState(seed).randint(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("split", [0, 1, 255, 65536, 70000])
def test_crc32_combine_equals_zlib_on_split_buffers(split):
    from cineflow.deflate import crc32_combine
    data = _rand_bytes(70000, 3)
    a, b = data[:split], data[split:]
    assert crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)
    assert crc32_combine(zlib.crc32(b), zlib.crc32(a), len(a)) == zlib.crc32(b + a)
    assert crc32_combine(0, 0, 0) == 0 and crc32_combine(zlib.crc32(a), 0, 0) == zlib.crc32(a)       # an empty second half, both empty
    with pytest.raises(ValueError):
        crc32_combine(1, 2, -1)


def test_pack_host_is_a_raw_deflate_stream_of_non_final_aligned_chunks():
    from cineflow import deflate
    data = _rand_bytes(1000, 1) + bytes(80000) + _rand_bytes(17, 2)
    p = deflate.pack_host(data)
    assert zlib.decompress(p.body + deflate.FINAL_BLOCK, -15) == data and p.crc == zlib.crc32(data) and p.size == len(data)
    assert p.body.endswith(b"\x00\x00\xff\xff")
    assert deflate.pack_host(b"") == deflate.Packed(b"", 0, 0)
    assert zlib.decompress(deflate.FINAL_BLOCK, -15) == b""


def _arrays():
    rs = np.random.RandomState(5)
    return {"data": rs.randn(3, 40, 33).astype(np.float32), "softmax": rs.rand(4, 9, 50, 21).astype(np.float16),
            "seg": (rs.rand(70000) * 4).astype(np.uint8), "idx": np.arange(-5, 12, dtype=np.int64), "flag": rs.rand(7, 3) > 0.5,
            "empty": np.zeros((0, 4), np.float32), "scalar": np.float64(2.5), "big_header_prefix": np.zeros((1,) * 20, np.int16)}


def test_npz_container_loads_in_numpy_and_zipfile(tmp_path):
    from cineflow import deflate
    arrays = _arrays()
    members = {k: deflate.npy_member(v, packer=deflate.pack_host) for k, v in arrays.items()}
    path = str(tmp_path / "case")
    deflate.write_npz(path, members)                      # numpy's rule: .npz is appended
    with np.load(path + ".npz") as z:
        assert sorted(z.files) == sorted(arrays)
        for k, v in arrays.items():
            got = z[k]
            assert got.dtype == np.asarray(v).dtype and got.shape == np.asarray(v).shape and got.tobytes() == np.asarray(v).tobytes(), k
    with zipfile.ZipFile(path + ".npz") as z:
        assert z.testzip() is None
        assert [i.filename for i in z.infolist()] == [k + ".npy" for k in arrays]
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
    buf = io.BytesIO()
    deflate.write_npz(buf, members)
    assert buf.getvalue() == open(path + ".npz", "rb").read() == deflate.npz_bytes(members)       # no clock in the file
    # one 0-byte array alone
    deflate.write_npz(str(tmp_path / "nothing.npz"), {"data": deflate.npy_member(np.zeros((0,), np.float32), packer=deflate.pack_host)})
    assert np.load(str(tmp_path / "nothing.npz"))["data"].shape == (0,)


def test_npy_header_is_numpys():
    from cineflow import deflate
    a = np.zeros((3, 5, 7), np.float16)
    f = io.BytesIO()
    np.save(f, a)
    assert f.getvalue().startswith(deflate.npy_header(a.shape, a.dtype))
    assert len(deflate.npy_header(a.shape, a.dtype)) + a.nbytes == len(f.getvalue())


def test_gzip_member_and_nifti_reader(tmp_path):
    from cineflow import deflate, nifti
    vol = (np.random.RandomState(2).rand(5, 31, 18) * 4).astype(np.uint8)
    geo = ((0.7, 0.8, 2.5), (1.0, -2.0, 3.0), (0, 1, 0, -1, 0, 0, 0, 0, 1))
    hdr = nifti.nifti_header(vol.shape, vol.dtype, *geo)
    assert len(hdr) == 352
    blob = deflate.gzip_bytes(hdr, deflate.pack_host(vol.tobytes()))
    assert gzip.decompress(blob) == hdr + vol.tobytes()
    path = str(tmp_path / "seg.nii.gz")
    with open(path, "wb") as f:
        f.write(blob)
    got, props = nifti.read_nifti(path)
    ref_path = str(tmp_path / "ref.nii.gz")
    nifti.write_nifti(ref_path, vol, *geo)                # the default route: untouched, and the same content
    ref, ref_props = nifti.read_nifti(ref_path)
    assert got.dtype == vol.dtype and np.array_equal(got, vol) and np.array_equal(ref, vol) and props == ref_props
    assert gzip.decompress(open(ref_path, "rb").read()) == gzip.decompress(blob)
    # a prefix longer than one stored block, and no data at all
    long_prefix = _rand_bytes(70000, 9)
    assert gzip.decompress(deflate.gzip_bytes(long_prefix, deflate.pack_host(b""))) == long_prefix
    assert gzip.decompress(deflate.gzip_bytes(b"", deflate.pack_host(b""))) == b""


def test_compress_keyword_is_checked():
    from cineflow import deflate, nifti
    assert deflate.check_compress("zlib") == "zlib" and deflate.check_compress("device") == "device"
    with pytest.raises(ValueError):
        deflate.check_compress("gpu")
    with pytest.raises(ValueError):
        nifti.write_nifti("/nonexistent/x.nii.gz", np.zeros((2, 2, 2), np.uint8), compress="lz4")


def test_deflate_argument_checks_need_no_gpu():
    """cf_deflate / cf_crc32 refuse on the host, before any launch, with made-up addresses that are never read."""
    from cineflow import _lib
    h = _lib.lib()
    a = 1 << 20
    CH = h.cf_deflate_chunk_bytes()
    assert 0 < CH <= 32768
    n = 3 * CH + 1
    cap, ws = h.cf_deflate_bound(n), h.cf_deflate_workspace_bytes(n)
    err = h.cf_last_error
    for args in ((None, n, a, cap, a, ws, a), (a, n, None, cap, a, ws, a), (a, n, a, cap, None, ws, a), (a, n, a, cap, a, ws, None)):
        assert h.cf_deflate(*args, None) == -1 and err() == b"cf_deflate: null pointer", args
    assert h.cf_deflate(a, -1, a, cap, a, ws, a, None) == -1 and b"negative" in err()
    assert h.cf_deflate(a, n, a, cap - 1, a, ws, a, None) == -1 and b"cf_deflate_bound" in err()
    assert h.cf_deflate(a, n, a, cap, a, ws - 1, a, None) == -1 and b"workspace" in err()
    assert h.cf_deflate(a, n, a, cap, a + 4, ws, a, None) == -1 and b"aligned" in err()
    cws = h.cf_crc32_workspace_bytes(n)
    for args in ((None, n, a, cws, a), (a, n, None, cws, a), (a, n, a, cws, None)):
        assert h.cf_crc32(*args, None) == -1 and err() == b"cf_crc32: null pointer", args
    assert h.cf_crc32(a, -5, a, cws, a, None) == -1 and b"negative" in err()
    assert h.cf_crc32(a, n, a, cws - 1, a, None) == -1 and b"workspace" in err()
    assert h.cf_crc32(a, n, a + 1, cws, a, None) == -1 and b"aligned" in err()


def test_deflate_bound_is_monotone_and_covers_stored_blocks():
    from cineflow import _lib
    h = _lib.lib()
    CH = h.cf_deflate_chunk_bytes()
    assert h.cf_deflate_bound.restype is ctypes.c_long and h.cf_deflate_workspace_bytes.restype is ctypes.c_long
    sizes = [0, 1, 2, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 7, 10 ** 6, 5 * 10 ** 6 + 3, 2 ** 31 + 5, 2 ** 33]
    prev = prev_ws = -1
    for n in sizes:
        b, w = h.cf_deflate_bound(n), h.cf_deflate_workspace_bytes(n)
        assert b >= n + 5 * -(-n // CH) and b >= prev and w >= prev_ws and w > 0, n
        prev, prev_ws = b, w
    assert h.cf_deflate_bound(0) == 0 and h.cf_deflate_bound(-1) == -1 and h.cf_deflate_workspace_bytes(-1) == -1
    assert h.cf_crc32_workspace_bytes(-1) == -1 and h.cf_crc32_workspace_bytes(0) > 0


def test_kernel_text_on_the_host_against_zlib(tmp_path):
    """tools/deflate_hostcheck.cpp compiles csrc/deflate_core.h, the text the device runs, for one host thread: every fixture's stream
    must inflate to its source under zlib and every folded CRC must equal zlib's."""
    # a host compiler is always there (the library's own hipcc at the least): without this program no CPU test holds the kernel's text
    # to an exact oracle, so a missing compiler or zlib header fails the test instead of skipping it
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    cmd = [cxx, "-O2", "-std=c++17"] if cxx else [hipcc, "-x", "c++", "-O2", "-std=c++17"]
    exe = str(tmp_path / "deflate_hostcheck")
    built = subprocess.run(cmd + [os.path.join(ROOT, "tools", "deflate_hostcheck.cpp"), "-lz", "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    sample = tmp_path / "sample.bin"
    sample.write_bytes(_rand_bytes(5000, 4) * 9 + bytes(40000))
    r = subprocess.run([exe, str(sample)], capture_output=True, text=True)
    assert r.returncode == 0 and "all streams inflate" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout and r.stdout.count("Kraft complete ok") == 4            # the 15- and 7-bit limits on Fibonacci weights
    # the stream it wrote for the sample, read by Python's zlib
    assert zlib.decompress((tmp_path / "sample.bin.deflate").read_bytes(), -15) == sample.read_bytes()
