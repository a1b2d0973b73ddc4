"""The skip projection of a residual-encoder stage -- a bias-free (1,1,1) convolution at stride (sd, s, s) -- on two routes, and one
FabiansUNet3D forward:

    composed  Conv3d._forward_composed: the volume permuted to [B, D, C, H, W], one 2-D 1x1 launch per sample, the result permuted back
    native    cf_conv3d_pw_f16s (csrc/conv3d_pw_f16s.hip) through Conv3d.forward with the InstanceNorm statistics from its epilogue (the
              composed route leaves them to a statistics pass that is NOT counted here)

Shapes: the projections of nnUNetTrainerV2_ResencUNet at trainer width on one 128^3 patch -- 32 -> 64 at 128^3, 64 -> 128 at 64^3,
128 -> 256 at 32^3, 256 -> 320 at 16^3, 320 -> 320 at 8^3 -- each at stride (2,2,2) and (1,2,2).  Then one forward of FabiansUNet3D(base 32,
blocks (1,2,3,4,4,4), seeded weights) on that patch, with the projections native and with the probe answering 0 (composed).

Every figure is the median of 20 samples after 5 warm-up samples; a sample is a pair of device events around `--calls` back-to-back calls;
the two routes of a case alternate sample by sample.  The outputs of both routes are compared once per case.

One worker process opens the GPU and runs the cases in order; this process never touches the GPU: it reads the worker's lines and ends the
worker -- and the run -- when a case takes longer than its own time limit (`--case_timeout` seconds, the network case four times that).

    python tools/resenc_bench.py [--calls 10] [--case_timeout 60] [--out FILE]      the table, then one JSON line per case"""
import argparse
import json
import os
import queue
import statistics
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cardiac-segmentation-optical-flow_amd"))

WIDTHS = [(32, 64, 128), (64, 128, 64), (128, 256, 32), (256, 320, 16), (320, 320, 8)]          # (cin, cout, edge of the input cube)
STRIDES = [(2, 2, 2), (1, 2, 2)]
NET = dict(base=32, blocks_encoder=(1, 2, 3, 4, 4, 4), blocks_decoder=(1, 1, 1, 1, 1), patch=128, classes=4)
WARMUP, SAMPLES = 5, 20


def cases():
    out = [("pw", cin, cout, n, st) for cin, cout, n in WIDTHS for st in STRIDES]
    return out + [("net",)]


def _samples(torch, fns, calls):
    """median seconds per call of each function: WARMUP + SAMPLES rounds, the functions alternating inside a round"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = [[] for _ in fns]
    for r in range(WARMUP + SAMPLES):
        for i, fn in enumerate(fns):
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                t[i].append(e0.elapsed_time(e1) * 1e-3 / calls)
    return [statistics.median(v) for v in t]


def worker(calls):
    import torch
    assert torch.cuda.is_available(), "resenc_bench needs a GPU"
    from cineflow import ops
    from cineflow.models import FabiansUNet3D
    from cineflow.nn import Conv3d
    from cineflow.weights import seeded_state_dict
    dev = torch.device("cuda:0")
    for idx, case in enumerate(cases()):
        print(json.dumps({"start": idx}), flush=True)
        if case[0] == "pw":
            _, cin, cout, n, st = case
            x = torch.randn((1, cin, n, n, n), generator=torch.Generator().manual_seed(idx)).to(dev)
            m = Conv3d(cin, cout, (1, 1, 1), st, bias=False)
            m.load_state_dict(seeded_state_dict(m.state_shapes(), 7), dev)
            assert ops.conv3d_pw_f16s_ok(1, cin, n, n, n, cout, st), "the probe declines the case: nothing native to time"
            y_n, ws = m(x, stats_groups=cout)
            y_c = m._forward_composed(x)
            assert ws is not None
            diff = float((y_n - y_c).abs().max())
            t_n, t_c = _samples(torch, [lambda: m(x, stats_groups=cout), lambda: m._forward_composed(x)], calls)
            do, ho = (n - 1) // st[0] + 1, (n - 1) // st[1] + 1
            # the bytes the layer cannot avoid: the 32-byte sectors of the sampled rows (every column of a row at s = 2 shares its sectors) + the output
            least = 4 * (cin * do * ho * n + cout * do * ho * ho)
            print(json.dumps({"case": "%d->%d @%d^3 stride %s" % (cin, cout, n, st), "native_us": round(t_n * 1e6, 1), "composed_us": round(t_c * 1e6, 1),
                              "composed_over_native": round(t_c / t_n, 2), "max_abs_diff": diff, "native_least_bytes_GBs": round(least / t_n / 1e9, 1)}),
                  flush=True)
            del x, m, y_n, y_c
        else:
            pool = [[1, 1, 1]] + [[2, 2, 2]] * (len(NET["blocks_encoder"]) - 1)
            net = FabiansUNet3D(1, NET["base"], NET["blocks_encoder"], pool, [[3, 3, 3]] * len(pool), NET["classes"], NET["blocks_decoder"])
            net.load_state_dict(seeded_state_dict(net.state_shapes(), 3), dev)
            p = NET["patch"]
            x = torch.randn((1, 1, p, p, p), generator=torch.Generator().manual_seed(99)).to(dev)
            real = ops.conv3d_pw_f16s_ok

            def composed():
                ops.conv3d_pw_f16s_ok = lambda *a: False
                try:
                    return net(x)
                finally:
                    ops.conv3d_pw_f16s_ok = real

            diff = float((net(x) - composed()).abs().max())
            t_n, t_c = _samples(torch, [lambda: net(x), composed], 1)
            print(json.dumps({"case": "FabiansUNet3D base %d blocks %s @%d^3" % (NET["base"], NET["blocks_encoder"], p), "native_us": round(t_n * 1e6, 1),
                              "composed_us": round(t_c * 1e6, 1), "composed_over_native": round(t_c / t_n, 3), "max_abs_diff": diff}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"done": True}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--case_timeout", type=float, default=60.0)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.calls)
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls)], stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in proc.stdout] + [lines.put(None)], daemon=True).start()
    all_cases, rows, limit, failed = cases(), [], 4 * a.case_timeout, None          # the first limit covers the import and the first case
    while True:
        try:
            ln = lines.get(timeout=limit)
        except queue.Empty:
            failed = "a case ran past its time limit of %.0f s: worker ended, nothing more started" % limit
            proc.kill()
            break
        if ln is None:
            break
        rec = json.loads(ln)
        if "start" in rec:
            limit = a.case_timeout * (4 if all_cases[rec["start"]][0] == "net" else 1)
        elif "case" in rec:
            rows.append(rec)
    rc = proc.wait()
    if failed is None and (rc != 0 or len(rows) != len(all_cases)):
        failed = "the worker ended with status %d after %d of %d cases" % (rc, len(rows), len(all_cases))
    table = ["%-52s %12s %12s %10s %12s" % ("case (median of %d after %d warm-ups)" % (SAMPLES, WARMUP), "native us", "composed us", "comp/nat", "max|diff|")]
    table += ["%-52s %12.1f %12.1f %10.2f %12.2e" % (r["case"], r["native_us"], r["composed_us"], r["composed_over_native"], r["max_abs_diff"]) for r in rows]
    if failed:
        table.append("INCOMPLETE: " + failed)
    text = "\n".join(table + [json.dumps(r) for r in rows]) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
