"""cf_deflate + cf_crc32 on the device against zlib on 16 host threads, on the arrays the folder commands compress.

Fixtures (seeded): at 12 x 256 x 224, a float32 cine-like image (sin(y/17) + cos(x/23) + 0.1 noise, a zero frame), the float32 label volume of
concentric discs 0-3, uniform random bytes of the same size, the same labels as uint8 (what a .nii.gz holds), and a (4, 10, 256, 216) fp16
softmax (blocky, tools/ensemble_bench.py's).

Device: the two calls back to back on one stream into buffers allocated once, `--iters` repetitions between two events after `--warmup`
repetitions; GB/s = input bytes / mean time.  The read-back of the compressed bytes is timed separately (host clock, synchronised).
Host: zlib.compress of the same bytes on 16 threads at once (each thread compresses the whole buffer; zlib releases the interpreter
lock), level 6 for what goes into .npz files and level 2 for the uint8 labels of a .nii.gz -- the levels the default route uses;
GB/s = 16 x input bytes / wall time, best of three.  Sizes: device stream, zlib level 6, level 1 (and level 2 for the .nii.gz case).

    python tools/deflate_bench.py [--iters 20] [--warmup 3] [--small]      one JSON line per fixture"""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def fixtures(small):
    import numpy as np
    from ensemble_bench import blocky_softmax
    Z, Y, X = (3, 64, 56) if small else (12, 256, 224)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    img = (np.sin(y / 17.0) + np.cos(x / 23.0) + 0.1 * np.random.RandomState(0).randn(Z, Y, X)).astype(np.float32)
    img[:, :Y // 6, :] = 0
    img[:, :, :X // 7] = 0
    r = np.hypot(y - Y / 2, x - X / 2)
    lab = np.zeros((Z, Y, X), np.float32)
    for k, rad in enumerate((0.35, 0.25, 0.12)):
        lab[r < rad * Y] = k + 1
    soft = blocky_softmax(4, (4, 32, 27) if small else (10, 256, 216), 71).astype(np.float16)
    return [("image_f32", img, 6), ("labels_f32", lab, 6), ("random_bytes", np.random.RandomState(1).randint(0, 256, img.nbytes, dtype=np.uint8), 6),
            ("softmax_f16", soft, 6), ("labels_u8_niigz", lab.astype(np.uint8), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "deflate_bench needs a GPU"
    from cineflow import _lib, ops
    h = _lib.lib()
    for name, arr, level in fixtures(a.small):
        raw = arr.tobytes()
        n = len(raw)
        t = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
        out = torch.empty(ops.deflate_bound(n), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(h.cf_deflate_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        cws = torch.empty(int(h.cf_crc32_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        nb = torch.zeros(1, dtype=torch.int64, device="cuda")
        crc = torch.zeros(1, dtype=torch.int64, device="cuda")

        def both():
            ops.deflate(t, out=out, ws=ws, out_bytes=nb)
            ops.crc32(t, ws=cws, crc=crc)

        for _ in range(a.warmup):
            both()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            both()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.iters
        t0 = time.perf_counter()
        k = int(nb.cpu())
        stream = out[:k].cpu().numpy().tobytes() + b"\x03\x00"
        back_ms = (time.perf_counter() - t0) * 1e3
        ok = zlib.decompress(stream, -15) == raw and (int(crc.cpu()) & 0xFFFFFFFF) == zlib.crc32(raw)

        best = None
        with ThreadPoolExecutor(16) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                sizes = list(pool.map(lambda _i: len(zlib.compress(raw, level)), range(16)))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        one = time.perf_counter()
        zlib.compress(raw, level)
        one = time.perf_counter() - one
        print(json.dumps({"fixture": name, "shape": list(arr.shape), "dtype": str(arr.dtype), "bytes": n, "inflates_and_crc_equal": bool(ok),
                          "device_ms": round(dev_ms, 4), "device_GBps": round(n / dev_ms / 1e6, 3), "readback_ms": round(back_ms, 3),
                          "zlib_level": level, "zlib_16_threads_GBps": round(16 * n / best / 1e9, 4), "zlib_1_thread_ms": round(one * 1e3, 2),
                          "size_device": len(stream), "size_zlib_level": sizes[0], "size_zlib_6": len(zlib.compress(raw, 6)),
                          "size_zlib_1": len(zlib.compress(raw, 1)), "device_over_zlib_6": round(len(stream) / len(zlib.compress(raw, 6)), 4),
                          "device_over_zlib_1": round(len(stream) / len(zlib.compress(raw, 1)), 4)}), flush=True)


if __name__ == "__main__":
    main()
