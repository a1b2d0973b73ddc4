"""Compressed .npz members and .nii.gz files from arrays that are still on the device.

The device compresses and checksums (ops.deflate / ops.crc32, csrc/deflate.hip); this module reads back the compressed bytes only and
writes the containers around them by hand: zip local headers, central directory and end record for `.npz`, the 10-byte gzip header and
the CRC-32 / ISIZE trailer for `.nii.gz`.  What the host adds in front of the device's data -- the `.npy` header of a member, the 352-byte
NIfTI header -- goes into the same DEFLATE stream as a stored block, and its CRC is joined with the device's by crc32_combine.

A DEFLATE stream cut into independently compressed chunks, each ending byte-aligned and non-final, is one valid raw-deflate stream
(pigz writes such streams); the two bytes 03 00, an empty final fixed-Huffman block, close it.  Every reader inflates it unchanged:
np.load, zipfile, gzip, nifti.read_nifti.  The files differ from zlib's in bytes and size, never in content; the same arrays give the
same file bytes on every run (the zip entries carry a fixed date, not the clock).

`compress="device"` on the writers of this package selects this route; the default `"zlib"` does not touch it.
"""
import collections
import os
import struct
import zlib

import numpy as np

COMPRESS_CHOICES = ("zlib", "device")
FINAL_BLOCK = b"\x03\x00"             # BFINAL 1, BTYPE 01, end-of-block: the empty final block that closes a stream of non-final ones
_POLY = 0xEDB88320
_U32 = 0xFFFFFFFF

# the compressed form of an array's bytes: body = non-final DEFLATE blocks ending on a byte boundary, crc / size of the bytes they inflate to
Packed = collections.namedtuple("Packed", "body crc size")
# one .npy member: the np.lib.format header (host bytes) and the packed array data
Member = collections.namedtuple("Member", "header packed")


def check_compress(compress):
    if compress not in COMPRESS_CHOICES:
        raise ValueError("compress must be one of %s, got %r" % (COMPRESS_CHOICES, compress))
    return compress


# ------------------------------------------------------------------------------------------------ CRC-32 arithmetic
def _gf_mul(a, b):
    """a(x) b(x) mod the CRC-32 polynomial, reflected: bit 31 is x^0 (zlib's multmodp)"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _x_pow_8n(n):
    sq, p, n = 1 << 30, 1 << 31, 8 * int(n)
    while n:
        if n & 1:
            p = _gf_mul(sq, p)
        sq = _gf_mul(sq, sq)
        n >>= 1
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(a + b) from zlib.crc32(a), zlib.crc32(b) and len(b)"""
    if len_b < 0:
        raise ValueError("len_b is negative")
    return (_gf_mul(_x_pow_8n(len_b), crc_a & _U32) ^ crc_b) & _U32


# ------------------------------------------------------------------------------------------------ packing
def _device_tensor(t):
    import torch
    if torch.is_tensor(t):
        if not t.is_cuda:
            raise ValueError("deflate: a tensor must live on the device (numpy arrays are uploaded)")
        return t
    a = np.ascontiguousarray(np.asarray(t))
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()        # (bytes: every dtype uploads, bool and float16 included)


def pack(t):
    """Compress and checksum a device tensor's bytes on the device; read back the stream and two numbers -> Packed."""
    import torch
    from . import ops
    t = _device_tensor(t)
    n = t.numel() * t.element_size()
    if n == 0:
        return Packed(b"", 0, 0)
    out, out_bytes = ops.deflate(t)
    crc = ops.crc32(t)
    k, c = (int(v) for v in torch.cat([out_bytes, crc]).cpu())
    return Packed(out[:k].cpu().numpy().tobytes(), c & _U32, n)


def pack_host(data, chunk=32768, strategy=zlib.Z_DEFAULT_STRATEGY, level=1):
    """The host stand-in for the kernel: zlib raw deflate per chunk, each ended with a sync flush.  Same shape of stream, same contract."""
    data = bytes(data)
    parts = []
    for i in range(0, len(data), chunk):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        parts.append(c.compress(data[i:i + chunk]) + c.flush(zlib.Z_SYNC_FLUSH))
    return Packed(b"".join(parts), zlib.crc32(data) & _U32, len(data))


def _stored(data):
    """data as non-final stored blocks (an empty input gives no block)"""
    out = []
    for i in range(0, len(data), 65535):
        part = data[i:i + 65535]
        out.append(struct.pack("<BHH", 0, len(part), len(part) ^ 0xFFFF) + part)
    return b"".join(out)


def _stream(prefix, packed):
    """-> (complete raw-deflate stream of prefix + data, its CRC-32, its uncompressed size)"""
    return (_stored(prefix) + packed.body + FINAL_BLOCK, crc32_combine(zlib.crc32(prefix), packed.crc, packed.size), len(prefix) + packed.size)


def deflate_raw(t):
    """A complete raw-deflate stream (zlib.decompress(s, -15)) of a contiguous device tensor's bytes."""
    return pack(t).body + FINAL_BLOCK


def crc32(t):
    """zlib.crc32 of a device tensor's bytes, computed on the device."""
    from . import ops
    t = _device_tensor(t)
    return int(ops.crc32(t).cpu()) & _U32 if t.numel() else 0


# ------------------------------------------------------------------------------------------------ .npz
_NP_OF_TORCH = {"torch.float32": np.float32, "torch.float16": np.float16, "torch.float64": np.float64, "torch.uint8": np.uint8, "torch.int8": np.int8,
                "torch.int16": np.int16, "torch.int32": np.int32, "torch.int64": np.int64, "torch.bool": np.bool_}


def numpy_dtype(t):
    """the numpy dtype of a tensor or array"""
    import torch
    if torch.is_tensor(t):
        if str(t.dtype) not in _NP_OF_TORCH:
            raise ValueError("deflate: no .npy dtype for %s" % t.dtype)
        return np.dtype(_NP_OF_TORCH[str(t.dtype)])
    return np.asarray(t).dtype


def npy_header(shape, dtype):
    """the bytes np.save writes in front of a C-order array of this shape and dtype"""
    import io
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, {"descr": np.lib.format.dtype_to_descr(np.dtype(dtype)), "fortran_order": False,
                                             "shape": tuple(int(s) for s in shape)})
    return f.getvalue()


def npy_member(value, packer=None):
    """value: a device tensor or a numpy array (uploaded) -> Member.  This is the device visit: the compressed bytes are on the host
    afterwards, and write_npz needs no device.  packer: pack_host in tests that have no device."""
    import torch
    value = value if torch.is_tensor(value) else np.asarray(value)
    dtype = numpy_dtype(value)
    if dtype.hasobject:
        raise ValueError("deflate: object arrays are not written")
    shape = tuple(value.shape)
    if packer is None:
        return Member(npy_header(shape, dtype), pack(value))
    a = value.cpu().numpy() if torch.is_tensor(value) else np.ascontiguousarray(np.asarray(value))
    return Member(npy_header(shape, dtype), packer(a.tobytes()))


_DOS_DATE = (1980 - 1980) << 9 | 1 << 5 | 1           # 1980-01-01 00:00: the same arrays give the same file


def npz_bytes(members):
    """members: {name: Member} -> the bytes of a zip file with one deflated entry `<name>.npy` per member, in the dict's order."""
    out, central, offset = [], [], 0
    for name, m in members.items():
        fname = (name + ".npy").encode("utf-8")
        flags = 0x800 if any(b > 127 for b in fname) else 0
        stream, crc, size = _stream(m.header, m.packed)
        if max(size, len(stream), offset) >= _U32:
            raise OverflowError("member %s does not fit a zip entry without zip64" % name)
        local = struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, flags, 8, 0, _DOS_DATE, crc, len(stream), size, len(fname), 0) + fname
        central.append(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, flags, 8, 0, _DOS_DATE, crc, len(stream), size, len(fname), 0, 0, 0, 0, 0,
                                   offset) + fname)
        out += [local, stream]
        offset += len(local) + len(stream)
    cd = b"".join(central)
    if offset + len(cd) >= _U32 or len(members) >= 0xFFFF:
        raise OverflowError("the archive does not fit a zip file without zip64")
    return b"".join(out) + cd + struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(members), len(members), len(cd), offset, 0)


def _npz_path(file):
    if isinstance(file, (str, bytes, os.PathLike)):
        file = os.fspath(file)
        return file if file.endswith(".npz") else file + ".npz"       # (numpy's own rule)
    return None


def write_npz(file, members):
    """file: a path (".npz" is appended when missing, as numpy does) or a binary file object"""
    data = npz_bytes(members)
    path = _npz_path(file)
    if path is None:
        file.write(data)
        return
    with open(path, "wb") as f:
        f.write(data)


_ZIP32_ROOM = _U32 - (1 << 20)


def savez_compressed(file, **arrays):
    """np.savez_compressed with the compression done on the device.  Values: device tensors, or numpy arrays (uploaded).  A member whose
    sizes do not fit 32 bits goes through numpy's own writer (zip64), and the whole file with it."""
    import torch
    arrays = {k: (v if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    sizes = [int(np.prod(v.shape, dtype=np.int64)) * numpy_dtype(v).itemsize for v in arrays.values()]
    bound = sum(s + 5 * (s // 32768 + 1) + 256 for s in sizes)
    if bound >= _ZIP32_ROOM:
        np.savez_compressed(file, **{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()})
        return
    write_npz(file, {k: npy_member(v) for k, v in arrays.items()})


# ------------------------------------------------------------------------------------------------ gzip
def gzip_bytes(prefix_bytes, packed):
    """One gzip member that inflates to prefix_bytes + the packed data"""
    stream, crc, size = _stream(bytes(prefix_bytes), packed)
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + stream + struct.pack("<II", crc, size & _U32)


def gzip_member(prefix_bytes, t):
    """A gzip member of prefix_bytes (host) followed by a device tensor's bytes: the header and the prefix as a stored block, then the
    device's stream, 03 00, CRC-32 and ISIZE."""
    return gzip_bytes(prefix_bytes, pack(t))
