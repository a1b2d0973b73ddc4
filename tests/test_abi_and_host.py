"""CPU tests (no GPU): the C-ABI library loads and exports every symbol include/cineflow.h declares, the ctypes
signatures match the header, the host logic (steps, Gaussian, padding, crop arithmetic, chunk order, state_dict
layout, sharding) matches the oracle, and the product refuses to run without its HIP library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cineflow.h")


def _header_prototypes():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(cf_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        kinds = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    kinds.append("P")
                elif re.match(r"(const\s+)?long\b", a):
                    kinds.append("L")
                elif re.match(r"(const\s+)?float\b", a):
                    kinds.append("F")
                elif re.match(r"(const\s+)?double\b", a):
                    kinds.append("D")
                elif re.match(r"(const\s+)?int\b", a):
                    kinds.append("I")
                else:
                    raise AssertionError("unparsed argument %r of %s" % (a, name))
        protos[name] = kinds
    return protos


def test_library_exports_every_declared_symbol():
    from cineflow import _lib
    h = _lib.lib()
    protos = _header_prototypes()
    assert len(protos) >= 25
    for name in list(protos) + ["cf_last_error"]:
        assert hasattr(h, name), "symbol %s missing from libcineflow_hip.so" % name
    assert h.cf_version() >= 100


def test_ctypes_signatures_match_header():
    from cineflow import _lib
    protos = _header_prototypes()
    protos.pop("cf_version")
    kind = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_long: "L", ctypes.c_float: "F", ctypes.c_double: "D"}
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, argtypes in _lib.SIGNATURES.items():
        assert [kind[a] for a in argtypes] == protos[name], name


def test_argument_validation_needs_no_gpu():
    """Shape errors are caught on the host before any launch (returns CF_ERR_ARG with a message)."""
    from cineflow import _lib
    h = _lib.lib()
    rc = h.cf_warp_bilinear_2d(None, None, None, 1, 1, 8, 8, None)
    assert rc == -1 and b"null pointer" in h.cf_last_error()
    rc = h.cf_attention_cf(1, 0, 1, 0, 1, 0, 1, 1, 4, 8, 33, 32, None)
    assert rc == -1 and b"multiples of 32" in h.cf_last_error()
    rc = h.cf_group_norm(1, None, None, None, 1, 2, 12, 16, 8, 1e-5, 0, 0, 1, None)
    assert rc == -1


def test_conv2d_argument_checks_need_no_gpu():
    """cf_conv2d (csrc/conv.hip) refuses on the host, before any launch, what conv_igemm_f32_kernel is not built for: asked here with made-up
    addresses.  Each call differs from an acceptable one (1 x 4 x 8 x 8 -> 6 channels, 3x3, stride 1, pad 1) in the one argument named."""
    from cineflow import _lib
    h = _lib.lib()
    a = 4096
    good = dict(x1=a, C1=4, x2=None, C2=0, wt=a, w_bstride=0, bias=None, res=None, out=a, out_ctotal=6, out_coff=0, B=1, H=8, W=8, Cout=6,
                KH=3, KW=3, stride=1, pad_h=1, pad_w=1, act=0, alpha=1.0, stream=None)

    def refused(message, **change):
        args = dict(good, **change)
        assert list(args) == list(good)
        rc = h.cf_conv2d(*args.values())
        err = h.cf_last_error()
        assert rc == -1 and message in err, (change, rc, err)

    refused(b"bad kernel", KH=16, pad_h=8)
    refused(b"bad kernel", KW=16, pad_w=8)
    refused(b"bad kernel", KH=0)
    refused(b"bad kernel", stride=5)
    refused(b"bad kernel", stride=0)
    refused(b"bad kernel", pad_w=-1)
    refused(b"output channel slice out of range", out_coff=1)              # [1, 7) of 6 channels
    refused(b"output channel slice out of range", out_ctotal=5)
    refused(b"output channel slice out of range", out_coff=-1, out_ctotal=8)
    refused(b"empty output", H=2, pad_h=0)                                 # 2 rows under a 3-row kernel
    refused(b"empty output", W=1, pad_w=0)
    refused(b"bad channel split C1=4 C2=2", C2=2)                          # a second input of two channels and no pointer to it
    refused(b"bad channel split C1=0 C2=0", C1=0)
    refused(b"null pointer", x1=None)
    refused(b"null pointer", wt=None)
    refused(b"null pointer", out=None)
    refused(b"bad shape", Cout=0)
    refused(b"bad activation 6", act=6)
    # per-sample weights: a 64-pixel wave tile must not straddle two samples
    refused(b"per-sample weights need Ho*Wo % 64 == 0 (got 16)", w_bstride=4 * 9 * 6, stride=2)
    refused(b"per-sample weights need Ho*Wo % 64 == 0 (got 36)", w_bstride=4 * 9 * 6, pad_h=0, pad_w=0)
    # the transposed convolution's own checks
    assert h.cf_conv_transpose2d_k2s2(a, a, None, a, 6, 1, 1, 4, 8, 8, 6, None) == -1 and b"output channel slice out of range" in h.cf_last_error()
    assert h.cf_conv_transpose2d_k2s2(a, a, None, a, 6, 0, 1, 0, 8, 8, 6, None) == -1 and b"bad shape" in h.cf_last_error()
    assert h.cf_conv_transpose2d_k2s2(a, None, None, a, 6, 0, 1, 4, 8, 8, 6, None) == -1 and b"null pointer" in h.cf_last_error()


def test_direct_conv_argument_checks_need_no_gpu():
    """the probes of the direct small-channel kernels (csrc/conv_direct.hip, csrc/conv_stem.hip) on both sides of each of their limits, and
    the entry points' refusals -- a null or aliased pointer, a shape the probe declines -- which happen on the host before any launch: asked
    here with made-up addresses.  The kernels themselves: tests/test_gpu_direct_conv_chains.py."""
    from cineflow import _lib
    h = _lib.lib()
    ok2 = h.cf_conv2d_small_cout_norm2_ok                      # (B, Cin, H, W, Cout)
    assert [ok2(2, 64, 33, 65, c) for c in (0, 1, 4, 5)] == [0, 1, 1, 0]
    assert [ok2(b, 64, 33, 65, 2) for b in (0, 1, 65535, 65536)] == [0, 1, 1, 0]
    assert [ok2(2, c, 33, 65, 2) for c in (0, 1)] == [0, 1]
    assert [ok2(2, 64, 0, 65, 2), ok2(2, 64, 33, 0, 2)] == [0, 0]
    assert [ok2(1, 1, 1, w, 1) for w in (2 ** 29 - 1, 2 ** 29)] == [1, 0]              # 4 Cin H W < 2 GiB: 32-bit byte offsets into one sample
    assert [ok2(1, 64, 1024, w, 1) for w in (8191, 8192)] == [1, 0]
    assert [ok2(1, 1, hh, 1, 1) for hh in (32 * 65535, 32 * 65535 + 1)] == [1, 0]      # grid.y
    oks = h.cf_stem_block_ok                                   # (B, Cin, H, W, Cout, gn_groups)
    assert [oks(2, c, 33, 65, 64, 8) for c in (0, 1, 2, 3, 6, 7)] == [0, 1, 0, 0, 1, 0]
    assert [oks(2, 6, 33, 65, 64, g) for g in (-8, 0, 1, 64)] == [0, 0, 1, 1]
    assert [oks(2, 6, 33, 65, 128, 64), oks(2, 6, 33, 65, 65, 65), oks(2, 6, 33, 65, 130, 65)] == [1, 0, 0]      # at most 64 groups
    assert [oks(2, 6, 33, 65, 60, 8), oks(2, 6, 33, 65, 0, 1)] == [0, 0]               # groups divide Cout; Cout > 0
    assert [oks(b, 1, 33, 65, 64, 8) for b in (0, 1, 65535, 65536)] == [0, 1, 1, 0]
    assert [oks(1, 1, 1, w, 2, 1) for w in (2 ** 30 - 1, 2 ** 30)] == [1, 0]           # Cout H W < 2^31 elements in one output sample
    assert [oks(1, 1, hh, 1, 1, 1) for hh in (8 * 65535, 8 * 65535 + 1)] == [1, 0]     # grid.y
    a, b, c, d, e = 4096, 8192, 12288, 16384, 20480

    def refused(message, rc):
        err = h.cf_last_error()
        assert rc == -1 and message in err, (rc, err)

    # cf_conv2d_small_cin(x, weight, bias, out, B, Cin, H, W, Cout, K, gn_ws, gn_groups, stream)
    for x, w, out in ((None, b, c), (a, None, c), (a, b, None), (a, b, a)):
        refused(b"null or aliased pointer", h.cf_conv2d_small_cin(x, w, None, out, 1, 1, 8, 8, 6, 3, None, 0, None))
    refused(b"built for Cin 1, 2, 6", h.cf_conv2d_small_cin(a, b, None, c, 1, 3, 8, 8, 6, 3, None, 0, None))
    refused(b"built for Cin 1, 2, 6", h.cf_conv2d_small_cin(a, b, None, c, 1, 2, 8, 8, 6, 5, None, 0, None))
    refused(b"bad shape", h.cf_conv2d_small_cin(a, b, None, c, 1, 1, 8, 8, 0, 3, None, 0, None))
    for cout, groups in ((130, 65), (64, 0), (64, -8), (60, 8)):
        refused(b"bad GroupNorm statistics request", h.cf_conv2d_small_cin(a, b, None, c, 1, 1, 8, 8, cout, 3, d, groups, None))
    for cin, K, rows in ((1, 3, 32), (2, 3, 16), (6, 3, 8), (6, 1, 32)):               # grid.y of the instantiation that (Cin, K) selects
        refused(b"block rows", h.cf_conv2d_small_cin(a, b, None, c, 1, cin, rows * 65535 + 1, 1, 6, K, None, 0, None))
    # cf_conv2d_small_cout(x, weight, bias, res, out, B, Cin, H, W, Cout, stream)
    for x, w, out in ((None, b, c), (a, None, c), (a, b, None), (a, b, a)):
        refused(b"null or aliased pointer", h.cf_conv2d_small_cout(x, w, None, None, out, 1, 8, 8, 8, 2, None))
    refused(b"built for 1..4 output channels, got 0", h.cf_conv2d_small_cout(a, b, None, None, c, 1, 8, 8, 8, 0, None))
    refused(b"built for 1..4 output channels, got 5", h.cf_conv2d_small_cout(a, b, None, None, c, 1, 8, 8, 8, 5, None))
    refused(b"below 2 GiB", h.cf_conv2d_small_cout(a, b, None, None, c, 1, 1, 1, 2 ** 29, 2, None))
    refused(b"block rows", h.cf_conv2d_small_cout(a, b, None, None, c, 1, 1, 32 * 65535 + 1, 1, 2, None))
    # cf_conv2d_small_cout_norm2(y2, coef2, r, coefr, weight, bias, out, B, Cin, H, W, Cout, stream)
    good = [a, b, c, d, e, None, 24576]
    for k in (0, 1, 2, 3, 4, 6):
        refused(b"null or aliased pointer", h.cf_conv2d_small_cout_norm2(*[None if j == k else v for j, v in enumerate(good)], 1, 8, 8, 8, 2, None))
    for k in (0, 2):                                                                   # out is y2, out is r
        refused(b"null or aliased pointer", h.cf_conv2d_small_cout_norm2(*good[:6], good[k], 1, 8, 8, 8, 2, None))
    refused(b"built for 1..4 output channels", h.cf_conv2d_small_cout_norm2(*good, 1, 8, 8, 8, 5, None))
    refused(b"built for 1..4 output channels", h.cf_conv2d_small_cout_norm2(*good, 1, 1, 1, 2 ** 29, 2, None))
    # cf_stem_block(x, w3, b3, w1, b1, y, r, B, Cin, H, W, Cout, ws_y, ws_r, gn_groups, stream) and cf_stem_block_y, the same without r
    ptrs = dict(x=a, w3=b, b3=None, w1=c, b1=None, y=d, r=e)
    shape, ws = (1, 6, 8, 8, 64), dict(ws_y=24576, ws_r=28672)

    def stem(groups=8, shape=shape, with_r=True, **change):
        p, s = dict(ptrs, **{k: v for k, v in change.items() if k in ptrs}), dict(ws, **{k: v for k, v in change.items() if k in ws})
        if with_r:
            return h.cf_stem_block(*p.values(), *shape, *s.values(), groups, None)
        p.pop("r")
        return h.cf_stem_block_y(*p.values(), *shape, *s.values(), groups, None)

    for with_r in (True, False):
        for name in ("x", "w3", "w1", "y", "ws_y", "ws_r") + (("r",) if with_r else ()):
            refused(b"null pointer", stem(with_r=with_r, **{name: None}))
        refused(b"aliased pointers", stem(with_r=with_r, y=a))
        refused(b"aliased pointers", stem(with_r=with_r, ws_r=24576))
        for groups in (65, 0, 60, -65):
            refused(b"<= 64 statistics groups dividing Cout", stem(groups, with_r=with_r))
        refused(b"built for Cin 1 or 6", stem(shape=(1, 2, 8, 8, 64), with_r=with_r))
        refused(b"one output sample below 2^31 elements", stem(1, shape=(1, 1, 1, 2 ** 30, 2), with_r=with_r))
    refused(b"aliased pointers", stem(r=a))
    refused(b"aliased pointers", stem(r=d))


def test_corr_volume_route_probe_needs_no_gpu():
    """cf_corr_volume_route is host code: the dispatch of cf_corr_volume (0 generic, 1 persistent fp32, 2 f16 MFMA) on shape, alignment
    and the cf_corr_mfma_enable knob, asked here with made-up addresses"""
    from cineflow import _lib
    h = _lib.lib()
    a, m = 4096, 4096 + 4                                          # a 16-byte aligned and a misaligned address
    route = lambda cur, prev, C, H, W, radius, stride: h.cf_corr_volume_route(cur, prev, C, H, W, radius, stride)
    before = h.cf_corr_mfma_enable(1)
    try:
        for C, H, W, S in ((16, 8, 64, 1), (16, 16, 64, 2), (16, 32, 64, 4), (256, 64, 64, 1), (64, 256, 256, 4)):
            assert route(a, a, C, H, W, 4, S) == 2, (C, H, W, S)
            assert route(m, a, C, H, W, 4, S) == 0 and route(a, m, C, H, W, 4, S) == 0, (C, H, W, S)
            assert route(a, a, C, H, W, 3, S) == 0 and route(a, a, C, H, W, 4, 3) == 0
        for C, H, W, S in ((8, 8, 64, 1), (24, 8, 64, 1), (16, 8, 128 + 4, 1), (16, 7, 64, 1), (16, 8, 64, 2), (16, 16, 64, 4), (5, 9, 12, 2)):
            assert route(a, a, C, H, W, 4, S) == 1, (C, H, W, S)      # C % 16, W % 64, H % (8 S): the MFMA kernel declines, p7 takes it
        assert route(a, a, 16, 8, 66, 4, 1) == 0 and route(a, a, 5, 7, 9, 4, 2) == 0      # W % 4 != 0
        assert h.cf_corr_mfma_enable(0) == 1
        assert route(a, a, 16, 8, 64, 4, 1) == 1 and route(m, a, 16, 8, 64, 4, 1) == 0
    finally:
        h.cf_corr_mfma_enable(before)


def test_attention_route_probe_needs_no_gpu():
    """cf_attention_cf_route is host code: the dispatch of cf_attention_cf / cf_attention_cf_masked (0 attention_cf_kernel<d>, 1
    attention_cf_f16s_kernel<d>) on the head dimension and on whether every 8-key group of V is 16-byte aligned -- the pointer, the batch
    stride and the key count --, asked here with made-up addresses"""
    from cineflow import _lib
    h = _lib.lib()
    a = 4096                                                       # a 16-byte aligned address
    route = h.cf_attention_cf_route
    for Nk in (32, 64, 96, 1024):
        for v_bs in (4 * Nk, 64 * Nk, 192 * Nk, 64 * Nk + 4, 64 * Nk + 1024):      # multiples of 4 floats: every sample stays aligned
            assert v_bs % 4 == 0
            assert route(a, v_bs, 8, Nk) == 0, (v_bs, Nk)
            for d in (16, 32, 64):
                assert route(a, v_bs, d, Nk) == 1, (d, v_bs, Nk)
                for off in (4, 8, 12):                             # V one, two, three floats off
                    assert route(a + off, v_bs, d, Nk) == 0, (d, off, v_bs, Nk)
        for v_bs in (64 * Nk + 1, 64 * Nk + 2, 64 * Nk + 3, 64 * Nk + 5, 64 * Nk + 7):      # odd, and even but no multiple of 4: sample 1 is off
            for d in (8, 16, 32, 64):
                assert route(a, v_bs, d, Nk) == 0 and route(a + 4, v_bs, d, Nk) == 0, (d, v_bs, Nk)
    for Nk in (4, 12, 36):                                         # Nk % 8 != 0 (the launcher refuses these; the probe has the whole condition)
        for d in (8, 16, 32, 64):
            assert route(a, 64 * 40, d, Nk) == 0, (d, Nk)
    for d in (0, 4, 12, 24, 48, 128, -8):
        h.cf_attention_cf_route(a, 4096, 8, 32)
        assert route(a, 64 * 64, d, 64) == -1 and b"head dim %d unsupported" % d in h.cf_last_error(), d
        assert route(a + 4, 64 * 64 + 1, d, 64) == -1, d           # whatever the alignment
    # the launcher asks the probe: the same unsupported d fails there before anything is queued
    assert h.cf_attention_cf(a, 4096, a, 4096, a, 4096, a, 1, 1, 24, 32, 32, None) == -1 and b"head dim 24 unsupported" in h.cf_last_error()


def test_group_norm_route_plan_needs_no_gpu():
    """cf_group_norm_route is the plan launch_gn_stats and gn_apply_launch execute, as host code: the plan of every row of
    test_gpu_norm_routes.py (written out by hand in _norm_refs.py), asked with made-up addresses -- one 16-byte aligned, one 4 bytes off --,
    the lines either side of each row, and the error returns of every norm entry, none of which reaches a launch"""
    import _norm_refs as R
    from cineflow import _lib
    h = _lib.lib()
    a, m = 4096, 4096 + 4

    def plan(x, out, res, B, C, HW, groups):
        p = (ctypes.c_int * 8)()
        assert h.cf_group_norm_route(x, out, res, B, C, HW, groups, ctypes.addressof(p)) == 0, h.cf_last_error()
        return tuple(p)

    for row in R.STATS_ROWS:
        x = m if row.view else a
        assert plan(x, None, None, row.B, row.C, row.HW, row.groups)[:3] == row.plan, row.name
    for row in R.APPLY_ROWS:
        x, res = (m if row.view == "x" else a), (m if row.view == "res" else a)
        out = x if row.inplace else a
        assert plan(x, out, res, row.B, row.C, row.HW, row.groups) == row.plan, row.name
        if row.view != "res":
            assert plan(x, out, None, row.B, row.C, row.HW, row.groups) == row.plan, row.name
    # the statistics line: L = 4096 | 4100, a misaligned or odd L of any size, the clamp of segs at 64 and the last L below it
    assert plan(a, a, None, 1, 1, 4096, 1)[:3] == (0, 0, 1) and plan(a, a, None, 1, 1, 4100, 1)[:3] == (1, 1, 1)
    assert plan(m, a, None, 1, 1, 1 << 20, 1)[:3] == (0, 0, 1) and plan(a, a, None, 5, 1, (1 << 20) + 2, 1)[:3] == (0, 0, 2)
    assert plan(a, a, None, 1, 1, 64 * 8192, 1)[:3] == (1, 64, 64) and plan(a, a, None, 1, 1, 64 * 8192 + 4, 1)[:3] == (1, 64, 64)
    assert plan(a, a, None, 3, 1, 63 * 8192 + 4, 1)[:3] == (1, 64, 192) and plan(a, a, None, 3, 1, 63 * 8192, 1)[:3] == (1, 63, 189)
    # the apply line: HW = 2047 | 2048, every pointer's alignment on its own, the ppb clamp at HW = 8 | 9
    assert plan(a, a, a, 1, 3, 2047, 1)[3:] == (0, 0, 2, 2, 1) and plan(a, a, a, 1, 3, 2048, 1)[3:] == (1, 1, 1, 3, 0)
    for x, out, res in ((m, a, a), (a, m, a), (a, a, m)):
        assert plan(x, out, res, 1, 3, 2048, 1)[3:] == (1, 0, 2, 6, 0) and plan(x, out, res, 1, 3, 512, 1)[3:] == (0, 0, 8, 1, 3)
    assert plan(a, a, None, 1, 1030, 8, 1)[3:] == (0, 1, 512, 3, 6) and plan(a, a, None, 1, 1030, 9, 1)[3:] == (0, 0, 455, 3, 120)
    assert plan(a, a, None, 1, 1, 4096 * 4 + 4, 1)[3:] == (1, 1, 5, 5, 0)
    assert h.cf_group_norm_route(a, a, None, 2, 8, 36, 4, None) == 0                        # plan8 is nullable

    def err(rc, text):
        assert rc == -1 and text in h.cf_last_error(), (rc, h.cf_last_error())

    err(h.cf_group_norm_route(a, a, None, 2, 12, 16, 8, None), b"bad shape")                # groups does not divide C
    err(h.cf_group_norm_route(a, a, None, 1, 2, 1 << 30, 1, None), b"slab too large")
    err(h.cf_group_norm_stats(a, a, 2, 12, 16, 8, None), b"bad shape")
    err(h.cf_group_norm_stats(None, a, 2, 8, 16, 8, None), b"null pointer")
    err(h.cf_group_norm(a, None, None, None, a, 2, 12, 16, 8, 1e-5, 0, 0, a, None), b"bad shape")
    err(h.cf_group_norm(a, None, None, None, a, 2, 8, 16, 8, 1e-5, 1, 1, a, None), b"without residual")
    err(h.cf_group_norm_apply(a, None, None, None, a, 2, 12, 16, 8, 1e-5, 0, 0, a, None), b"bad shape")
    err(h.cf_group_norm_apply(a, None, None, None, a, 2, 8, 16, 8, 1e-5, 0, 2, a, None), b"without residual")
    err(h.cf_group_norm_apply(a, None, None, None, a, 2, 8, 16, 8, 1e-5, 6, 0, a, None), b"bad activation")
    err(h.cf_group_norm_apply_res_norm(a, None, None, a, a, 2, 8, 16, 8, 1e-5, 1, 0, a, a, None, None, None), b"needs a residual mode")
    err(h.cf_group_norm_apply_res_norm(a, None, None, None, a, 2, 8, 16, 8, 1e-5, 1, 1, a, a, None, None, None), b"null pointer")
    err(h.cf_group_norm_apply_res_norm(a, None, None, a, a, 2, 12, 16, 8, 1e-5, 1, 1, a, a, None, None, None), b"bad shape")
    err(h.cf_group_norm_coef(a, None, None, 2, 12, 16, 8, 1e-5, a, None), b"bad shape")
    err(h.cf_layer_norm_cf(a, a, a, a, 2, 0, 16, 1e-5, None), b"bad shape")
    err(h.cf_layer_norm_cf(a, None, a, a, 2, 8, 16, 1e-5, None), b"null pointer")
    err(h.cf_norm_head_1x1(a, a, 0.01, a, None, a, 2, 8, 18, 4, None), b"HW % 4 == 0")      # HW % 4
    err(h.cf_norm_head_1x1(a, a, 0.01, a, None, a, 2, 8, 16, 3, None), b"K=3")
    err(h.cf_norm_head_1x1(a, a, 0.01, a, None, a, 2, 1025, 16, 4, None), b"C=1025")
    err(h.cf_norm_head_1x1(a, a, -0.01, a, None, a, 2, 8, 16, 4, None), b"slope must be >= 0")
    err(h.cf_norm_head_1x1(m, a, 0.01, a, None, a, 2, 8, 16, 4, None), b"16-byte aligned")
    err(h.cf_norm_head_1x1(a, a, 0.01, a, None, m, 2, 8, 16, 4, None), b"16-byte aligned")


def test_conv2d_f16s_route_plan_needs_no_gpu():
    """cf_conv2d_f16s_route is the plan the f16-split launcher executes, as host code: the instantiation of every row of
    test_gpu_conv_f16s_routes.py in both product modes, and the conditions no GPU test can afford -- sub-batches, the 1024-workgroup and
    1024-tile lines, the stream knob, every decline of a deferred normalisation, and the limits that used to be found at launch."""
    from collections import namedtuple
    from cineflow import _lib
    from _conv_f16s_rows import CONVT_ROWS, NARROW_ROWS, PAD, PRE_ROWS, ROWS
    h = _lib.lib()
    Plan = namedtuple("Plan", "route tup terms nimg fused part")

    def route(B, C1, H, W, cout, k=(3, 3), stride=1, C2=0, lo1=0, lo2=0, prenorm=0, transposed=0, groups=0):
        plan = (ctypes.c_int * 15)()
        r = h.cf_conv2d_f16s_route(B, C1, C2, H, W, cout, k[0], k[1], stride, PAD[k][0], PAD[k][1], lo1, lo2, prenorm, transposed, groups, plan)
        assert r == plan[0] and r in (0, 1, 2), r
        return Plan(r, tuple(plan[1:11]), plan[11], plan[12], bool(plan[13]), plan[14])

    def declined(why, *a, **k):
        p = route(*a, **k)
        assert p.route == 0 and p.tup == (0,) * 10 and why in h.cf_last_error(), (a, k, p, h.cf_last_error())

    WL32, WL64 = (3, 3, 16, 1, 1, 2, 8, 1, 0, 1), (3, 3, 16, 2, 2, 2, 8, 1, 0, 1)
    knob, mode = h.cf_conv_stream_enable(1), h.cf_conv_terms(3)
    try:
        assert len(ROWS) + len(PRE_ROWS) + len(CONVT_ROWS) == 34 and len({r.tup for r in ROWS + PRE_ROWS}) == 30
        for terms in (3, 1):
            h.cf_conv_terms(terms)
            for r in ROWS + NARROW_ROWS:
                groups = 8 if r.Cout % 8 == 0 else r.Cout
                for g in (0, groups):
                    assert route(r.B, r.C, r.H, r.W, r.Cout, r.k, r.stride, lo1=4 if r.view else 0, groups=g) == \
                        (1, r.tup, terms, r.nimg, r.nimg == 1, r.B), (r, terms)
            for r in PRE_ROWS:
                assert route(r.B, r.C, r.H, r.W, r.Cout, prenorm=1, groups=r.Cout) == (1, r.tup, terms, 1, True, r.B), (r, terms)
            for r in CONVT_ROWS:
                assert route(r.B, r.Cin, r.H, r.W, r.Cout, (1, 1), transposed=1, groups=4) == (1, r.tup, terms, r.nimg, r.nimg == 1, r.B), (r, terms)
        h.cf_conv_terms(3)
        # sub-batches: a sample of 4000 x 32 x 64 floats is 31.25 MiB, 65 of them stay below 2 GiB; 127 samples are cut into the fewest parts
        # that fit, 2, made equal: 64 + 63 (a greedy cut: 65 + 62).  64 samples x 16 tiles reach the 1024 workgroups of the four-wave shape,
        # the 63 of the last part do not: asking with B = 63 names the eight-wave shape that part runs on.
        four, eight = (3, 3, 16, 4, 4, 2, 4, 1, 0, 0), (3, 3, 16, 4, 2, 2, 8, 1, 0, 0)
        assert route(65, 4000, 32, 64, 128) == (1, four, 3, 1, True, 65)
        assert route(127, 4000, 32, 64, 128) == (1, four, 3, 1, True, 64)
        assert route(63, 4000, 32, 64, 128) == (1, eight, 3, 1, True, 63)
        assert route(131, 4000, 32, 64, 128).part == 44          # ceil(131 / 3): three parts, the last one 43
        declined(b"unsupported configuration", 1, 2 ** 19, 32, 64, 128)          # one sample of the input at 4 GiB: the argument-level gate
        # 480 = 3 x 128 + 96 output channels on 32x32 maps: 8 tiles x 4 channel blocks per sample.  32 samples make the 1024 workgroups at which
        # the layer rides on the 128-channel four-wave shape; 31 keep the 64-channel one (weights through LDS)
        assert route(32, 40, 32, 32, 480) == (1, four, 3, 1, True, 32)
        assert route(31, 40, 32, 32, 480) == (1, WL64, 3, 1, True, 31)
        # the stream route: 3x3 / stride 1 to 32 or 64 channels, an even number of 16-channel chunks, >= 1024 tiles (8 rows x 32 at 64
        # channels, 16 rows x 32 at 32: 16 / 8 tiles per 64x64 sample).  Level 0 keeps conv_f16s_kernel, level 1 leaves it the 64-channel
        # layers with a deferred normalisation, level 2 takes every shape; the one-term mode is built in conv_f16s_kernel only
        stream = (2, (0,) * 10, 3, 1, True)
        PRE64 = WL64[:8] + (1, 1)
        for level in (0, 1, 2):
            h.cf_conv_stream_enable(level)
            on = level > 0
            assert route(64, 32, 64, 64, 64, groups=8) == (stream + (64,) if on else (1, WL64, 3, 1, True, 64)), level
            assert route(63, 32, 64, 64, 64, groups=8) == (1, WL64, 3, 1, True, 63), level
            assert route(128, 32, 64, 64, 32) == (stream + (128,) if on else (1, WL32, 3, 1, True, 128)), level
            assert route(127, 32, 64, 64, 32) == (1, WL32, 3, 1, True, 127), level
            assert route(64, 32, 64, 64, 64, prenorm=1) == (stream + (64,) if level == 2 else (1, PRE64, 3, 1, True, 64)), level
            assert route(128, 32, 64, 64, 32, prenorm=1) == (stream + (128,) if on else (1, WL32[:8] + (1, 1), 3, 1, True, 128)), level
            assert route(64, 40, 64, 64, 64).route == 1 and route(64, 32, 64, 64, 64, lo1=4).route == 1, level       # 3 chunks; misaligned
            h.cf_conv_terms(1)
            assert route(64, 32, 64, 64, 64) == (1, WL64, 1, 1, True, 64), level
            h.cf_conv_terms(3)
        h.cf_conv_stream_enable(1)
        # a deferred normalisation is declined, with the message the call fails with
        assert route(2, 40, 20, 36, 48, prenorm=1).tup == PRE64
        declined(b"not built for this layer shape", 2, 40, 20, 36, 48, C2=8, prenorm=1)
        declined(b"needs the vector staging path", 2, 40, 20, 36, 48, lo1=4, prenorm=1)
        declined(b"needs the vector staging path", 2, 40, 20, 34, 48, prenorm=1)             # W % 4 != 0
        declined(b"needs the vector staging path", 2, 40, 20, 36, 48, stride=2, prenorm=1)
        declined(b"needs the vector staging path", 2, 40, 20, 36, 48, k=(1, 1), prenorm=1)
        declined(b"not built for this layer shape", 2, 40, 32, 32, 128, prenorm=1)           # the eight-wave shape of the small launches
        # the limits that were found only at launch: the plan declines, and the call fails with the same message.  The calls get made-up
        # addresses, so each is made only after `declined` has asserted that the plan -- the one the call executes -- queues nothing.
        # One workgroup's output at 1 GiB is caught by the argument-level gate of the call, as before (the plan's own check is a backstop).
        a = 4096
        conv = lambda B, C, H, W, cout: h.cf_conv2d_f16s(a, C, None, 0, a, None, None, a, cout, 0, B, H, W, cout, 3, 3, 1, 1, 1, 0, 1.0, None, 0, None)
        # a one-column map taller than the staging budget was such a limit (Conv3d's composition ran into it on maps the 3-D probe leaves
        # to it): the plan gives its tile fewer rows instead, on both sides of the old line (84 rows at 3x3 / stride 1) and for every kernel
        # shape with a patch -- no narrow tall map of this grid is declined
        assert route(2, 8, 83, 1, 24) == route(2, 8, 84, 1, 24) == route(2, 8, 200, 1, 24) == (1, (3, 3, 16, 1, 1, 2, 4, 0, 0, 0), 3, 1, True, 2)
        for k, stride in (((3, 3), 1), ((3, 3), 2), ((1, 5), 1), ((5, 1), 1)):
            for W in (1, 2, 3, 4):
                for H in (60, 84, 130, 300, 513):
                    for cout in (24, 48, 128, 224):
                        assert route(3, 40, H, W, cout, k, stride).route == 1, (k, stride, H, W, cout, h.cf_last_error())
        declined(b"unsupported configuration", 1, 4, 4096, 4096, 16)                          # 16 x 4096 x 4096 floats = 1 GiB
        assert conv(1, 4, 4096, 4096, 16) == -1 and b"unsupported configuration for the f16-split kernel" in h.cf_last_error()
        declined(b"conv_f16s: LDS tile too large", 1, 14000, 4, 4, 24, prenorm=1)             # 3 x 14000 floats of coefficients beside the patch
        assert h.cf_conv2d_f16s_prenorm(a, 14000, a, 0.01, a, None, a, 1, 4, 4, 24, 1.0, None, 0, None) == -1
        assert h.cf_last_error() == b"conv_f16s: LDS tile too large"
        assert h.cf_conv2d_f16s_prenorm_ok(1, 14000, 4, 4, 24) == 0 and h.cf_conv2d_f16s_prenorm_ok(2, 40, 20, 36, 48) == 1
        # the plan names rows of the table only: no layer of a grid over every routing condition is declined for "a shape that is not built"
        n = 0
        for terms in (3, 1):
            h.cf_conv_terms(terms)
            for k, strides in (((3, 3), (1, 2)), ((1, 1), (1, 2)), ((1, 5), (1,)), ((5, 1), (1,))):
                for stride in strides:
                    for cout in (8, 32, 48, 64, 96, 128, 224, 256, 480):
                        for H, W in ((4, 5), (6, 12), (10, 8), (8, 12), (20, 36), (32, 32), (33, 45), (64, 64), (200, 1), (12, 40)):
                            for B in (1, 3, 11, 128):
                                for C2, lo1, pre in ((0, 0, 0), (13, 0, 0), (0, 4, 0), (0, 0, 1)):
                                    p = route(B, 40, H, W, cout, k, stride, C2=C2, lo1=lo1, prenorm=pre, groups=8)
                                    assert p.route or b"not built" not in h.cf_last_error().replace(b"not built for this layer shape", b""), (k, stride, cout, H, W, B)
                                    n += 1
        assert n == 2 * 6 * 9 * 10 * 4 * 4
    finally:
        h.cf_conv_stream_enable(knob)
        h.cf_conv_terms(mode)


def test_product_fails_loudly_without_library(monkeypatch):
    from cineflow import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcineflow_hip.so")
    with pytest.raises(_lib.CineflowLibraryError):
        _lib.lib()


def test_ops_reject_cpu_tensors():
    from cineflow import ops
    with pytest.raises(TypeError):
        ops.warp_bilinear(torch.zeros(1, 2, 8, 8), torch.zeros(1, 1, 8, 8))


# ---------------------------------------------------------------- host logic vs oracle
def test_host_steps_gaussian_padding_match_oracle():
    from cineflow import inference as inf
    from oracle import ops as OO
    rng = np.random.RandomState(1)
    for _ in range(500):
        dim = rng.choice((2, 3))
        patch = tuple(int(v) for v in rng.randint(16, 512, dim))
        image = tuple(max(int(rng.randint(p // 2, p * 6)), p) for p in patch)
        step = float(rng.uniform(0.05, 1))
        assert inf.compute_steps_for_sliding_window(patch, image, step) == OO.compute_steps_for_sliding_window(patch, image, step)
    assert inf.compute_steps_for_sliding_window((64, 130), (128, 260), 0.5) == [[0, 32, 64], [0, 65, 130]]
    assert np.array_equal(inf.get_gaussian((64, 48)), OO.get_gaussian((64, 48)))
    x = rng.randn(3, 50, 61).astype(np.float32)
    a, sa = inf.pad_nd_image(x, (64, 64), "constant", {"constant_values": 0}, True)
    b, sb = OO.pad_nd_image(x, (64, 64), "constant", {"constant_values": 0}, True)
    assert np.array_equal(a, b) and sa == sb
    a = inf.pad_nd_image(x, (32, 32))
    assert a is x


def test_processor_arithmetic_matches_oracle():
    from cineflow.inference import Processor
    from oracle.models import Processor as OP
    for crop, image in ((128, 224), (192, 384), (16, 40)):
        p, o = Processor(crop, image), OP(crop, image)
        rng = np.random.RandomState(2)
        for _ in range(200):
            c = (int(rng.randint(0, image)), int(rng.randint(0, image)))
            a, b = p.adjust_cropping_window(c), o.adjust_cropping_window(c)
            assert a["crop_indices"] == b["crop_indices"]
            assert a["padding_need"] == b["padding_need"].tolist()


def test_chunk_orders_match_torch_chunk():
    from cineflow.inference import chunk_orders
    for T in (2, 3, 4, 5, 12, 30, 31):
        idx = torch.arange(1, T)
        c1, c2 = (torch.chunk(idx, 2) + (torch.tensor([], dtype=torch.long),))[:2] if T > 2 else (idx, torch.tensor([], dtype=torch.long))
        want1 = [0] + c1.tolist()
        want2 = [0] + torch.flip(c2, dims=[0]).tolist()
        assert chunk_orders(T) == (want1, want2), T


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_layout_matches_oracle_and_reference_names():
    """The product modules declare exactly the reference's state_dict keys and shapes (via the oracle, whose
    strict load against the reference is checked in make_golden.py)."""
    from cineflow import models as PM
    from cineflow import nn as PN
    from oracle import models as OM
    red = dict(in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32])
    pairs = [
        (PM.SegFlowGaussian(image_size=64, d_model=32, dim_feedforward=64, motion_appearance=True, **red),
         OM.SegFlowGaussian(image_size=64, d_model=32, dim_feedforward=64, motion_appearance=True, **red)),
        (PM.SegFlowGaussian(image_size=64, d_model=32, dim_feedforward=48, motion_appearance=False, **red),
         OM.SegFlowGaussian(image_size=64, d_model=32, dim_feedforward=48, motion_appearance=False, **red)),
        (PM.SegFlowGaussian(image_size=256, motion_appearance=False, dim_feedforward=2048, raft=True),
         OM.SegFlowGaussian(image_size=256, motion_appearance=False, dim_feedforward=2048, raft=True)),
        (PM.ModelWrap(PM.OpticalFlowModelSuccessive(64, 1, **red), PM.OpticalFlowModelSuccessive(64, 6, **red)),
         OM.ModelWrap(OM.OpticalFlowModelSuccessive(64, 1, **red), OM.OpticalFlowModelSuccessive(64, 6, **red))),
        (PM.Generic_UNet(1, 8, 4, 3), OM.GenericUNet2D(1, 8, 4, 3)),
        (PM.Generic_UNet(1, 32, 4, 6), OM.GenericUNet2D(1, 32, 4, 6)),
        (PN.ConvGRUCell((8, 8), 32, 32), OM.ConvGRUCell((8, 8), 32, 32)),
    ]
    for prod, ora in pairs:
        assert prod.state_shapes() == _shapes(ora), type(prod).__name__


def test_full_width_parameter_counts():
    """SURVEY.md appendix A [measured]: 25 357 698 params for the video.yaml model, 25 267 906 for raft_config.yaml."""
    from cineflow import models as PM
    def count(m):
        return sum(int(np.prod(s)) for k, s in m.state_shapes().items() if not k.endswith("grid"))
    assert count(PM.SegFlowGaussian(image_size=256, motion_appearance=False, dim_feedforward=2048)) == 25357698
    assert count(PM.SegFlowGaussian(image_size=256, motion_appearance=True, dim_feedforward=3072)) == 25267906


def test_seeded_weights_are_deterministic_and_name_keyed():
    from cineflow.weights import seeded_state_dict
    a = seeded_state_dict({"x.conv1.weight": (4, 3, 3, 3), "x.norm1.weight": (4,), "m.grid": (1, 2, 4, 4)}, seed=3)
    b = seeded_state_dict({"x.norm1.weight": (4,), "x.conv1.weight": (4, 3, 3, 3)}, seed=3)
    assert "m.grid" not in a
    assert torch.equal(a["x.conv1.weight"], b["x.conv1.weight"]) and torch.equal(a["x.norm1.weight"], b["x.norm1.weight"])
    c = seeded_state_dict({"x.conv1.weight": (4, 3, 3, 3)}, seed=4)
    assert not torch.equal(a["x.conv1.weight"], c["x.conv1.weight"])
    assert abs(float(a["x.norm1.weight"].mean()) - 1.0) < 0.3


def test_shard_is_the_reference_partition():
    from cineflow.parallel import shard
    items = list(range(11))
    parts = [shard(items, r, 4) for r in range(4)]
    assert parts[1] == items[1::4]
    assert sorted(sum(parts, [])) == items


def test_properties_pkl_reader_rebuilds_plain_values_and_refuses_globals(tmp_path):
    """the voxelmorph_saver consumer reads <pkl_path>/<case>.pkl files another pipeline may have written -- nnU-Net property
    dicts (OrderedDict, lists, tuples, numpy arrays / scalars) load, any other global is refused before it is imported or called."""
    import collections
    import pickle
    from cineflow.voxelmorph_saver import load_plain_pickle
    props = collections.OrderedDict(original_size_of_raw_data=np.array([10, 256, 216]), original_spacing=np.array([10.0, 1.25, 1.25]),
                                    list_of_data_files=["a_0000.nii.gz"], itk_spacing=(1.25, 1.25, 10.0), crop_bbox=[[0, 10], [0, 256], [0, 216]],
                                    classes=np.array([0, 1, 2, 3], dtype=np.int16), size_after_cropping=(10, 256, 216), use_nonzero_mask_for_norm={0: False},
                                    padding_need=np.arange(40, dtype=np.int64).reshape(4, 10), voxelmorph_size_before=[256, 216, 10],
                                    a_scalar=np.float64(1.5), an_int_scalar=np.int32(7))
    ok = tmp_path / "ok.pkl"
    with open(ok, "wb") as f:
        pickle.dump(props, f)
    got = load_plain_pickle(str(ok))
    assert list(got.keys()) == list(props.keys())
    assert np.array_equal(got["padding_need"], props["padding_need"]) and got["a_scalar"] == 1.5 and got["itk_spacing"] == (1.25, 1.25, 10.0)

    class Evil:
        def __reduce__(self):
            import os
            return (os.system, ("echo pwned > %s" % (tmp_path / "pwned"),))

    bad = tmp_path / "bad.pkl"
    with open(bad, "wb") as f:
        pickle.dump({"padding_need": np.zeros((4, 1)), "x": Evil()}, f)
    with pytest.raises(pickle.UnpicklingError):
        load_plain_pickle(str(bad))
    assert not (tmp_path / "pwned").exists()


def test_conv_f16s_output_sample_limit_falls_back_to_fp32_kernel():
    """a destination buffer whose sample exceeds the epilogue's 32-bit store range makes f16s_dynamic_ok say no (the layer then
    takes the exact fp32 kernel) instead of raising from inside the library.  Host logic only."""
    from cineflow import ops

    class Fake:
        def __init__(self, shape):
            self.shape = shape

        def numel(self):
            n = 1
            for v in self.shape:
                n *= v
            return n
    x = Fake((1, 16, 4096, 4096))                                            # 1 GiB input sample: fine (< 2 GiB)
    assert ops.f16s_dynamic_ok(x, None, 3, out_sample_elems=8 * 4096 * 4096, out_hw=4096 * 4096)
    assert not ops.f16s_dynamic_ok(x, None, 3, out_sample_elems=16 * 4096 * 4096, out_hw=4096 * 4096)      # 1 GiB output sample
    assert not ops.f16s_dynamic_ok(Fake((1, 8, 16, 16)), None, 3, out_sample_elems=2 ** 25, out_hw=256)      # 8 images per workgroup


def test_packed_conv_objects_take_the_fp32_call_at_the_output_sample_limit(monkeypatch):
    """the same limit at every site: a convroute.PackedConv of a 1x1 layer and a PackedConvT (destination sample x4: the scatter) make the
    fp32 call when one sample of the destination buffer reaches 1 GiB and the f16 call one channel below it.  Host logic only: fake
    tensors, the ops launch functions replaced by recorders."""
    from cineflow import ops
    from cineflow.convroute import PackedConv, PackedConvT

    class Fake:
        def __init__(self, shape):
            self.shape = shape

        def numel(self):
            n = 1
            for v in self.shape:
                n *= v
            return n

        def data_ptr(self):
            return 0
    calls = []
    for name in ("conv2d_f16s", "conv2d", "conv2d_wino", "conv_transpose2d_k2s2_f16s", "conv_transpose2d_k2s2"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n) or _n)
    monkeypatch.setattr(ops, "CONV_MODE", "f16s")
    g = torch.Generator().manual_seed(0)
    conv = PackedConv(torch.randn(8, 16, 1, 1, generator=g), torch.randn(8, generator=g))
    x = Fake((1, 16, 4096, 4096))
    assert conv(x, out=Fake((1, 15, 4096, 4096)), out_coff=2) == "conv2d_f16s"           # 15 * 2^24 * 4 bytes < 1 GiB
    assert conv(x, out=Fake((1, 16, 4096, 4096)), out_coff=2) == "conv2d"                # 16 * 2^24 * 4 bytes = 1 GiB
    assert conv(x, out=Fake((1, 16, 4096, 4096)), stats_groups=8) == ("conv2d", None)
    up = PackedConvT(torch.randn(16, 8, 2, 2, generator=g), torch.randn(8, generator=g))
    x = Fake((1, 16, 2048, 2048))
    assert up(x, out=Fake((1, 15, 4096, 4096))) == "conv_transpose2d_k2s2_f16s"          # 15 * 4 * 2^22 * 4 bytes < 1 GiB
    assert up(x, out=Fake((1, 16, 4096, 4096))) == "conv_transpose2d_k2s2"
    assert up(Fake((1, 16, 16, 16)), out=Fake((1, 2 ** 15, 32, 32))) == "conv_transpose2d_k2s2"      # <= 256 pixels: 8 images per workgroup
    assert up(Fake((1, 16, 16, 16)), out=Fake((1, 2 ** 15 - 1, 32, 32))) == "conv_transpose2d_k2s2_f16s"
    assert calls == ["conv2d_f16s", "conv2d", "conv2d", "conv_transpose2d_k2s2_f16s", "conv_transpose2d_k2s2", "conv_transpose2d_k2s2",
                     "conv_transpose2d_k2s2_f16s"]


def test_wino_form_query_follows_the_route_level():
    """cf_conv2d_wino_form names the kernel form the dispatch picks (host code, no launch); cf_conv2d_wino_ok is `form != 0`.  A layer with
    few items: level 1 takes NTW 2 -- never NTW 4, which only the forced level 4 selects."""
    from cineflow import _lib, ops
    h = _lib.lib()
    prev = h.cf_conv_wino_enable(1)
    try:
        for level, form in ((0, 0), (1, 2), (2, 2), (4, 4), (8, 8)):
            h.cf_conv_wino_enable(level)
            assert ops.wino_form(2, 128, 0, 16, 32, 128) == form and ops.wino_ok(2, 128, 0, 16, 32, 128) == (form != 0), level
            assert ops.wino_form(2, 128, 0, 16, 48, 128) == 0 and not ops.wino_ok(2, 128, 0, 16, 48, 128)       # W = 48: no form
            assert ops.wino_form(2, 128, 0, 12, 32, 128) == (0 if level in (0, 4) else level if level > 1 else 2)   # H % 8 != 0: no NTW 4
    finally:
        h.cf_conv_wino_enable(prev)


# (B, C1, C2, H, W, Cout): few items per CU unless B = 64
_WINO_PLAN_SHAPES = (
    (2, 128, 0, 16, 32, 128),
    (2, 48, 0, 16, 32, 128),        # an odd number of 16-channel chunks: never the 16x16x32 form
    (2, 20, 28, 16, 32, 128),       # a split input: no deferred norm
    (2, 64, 0, 16, 32, 224),        # a last block of 96
    (2, 64, 0, 16, 32, 200),        # a last block of 72: no form
    (2, 64, 0, 16, 16, 128),        # W = 16: 16-column tiles
    (2, 64, 0, 16, 48, 128),        # W = 48: no tile width divides it
    (2, 64, 0, 12, 32, 128),        # H % 8 != 0: no NTW 4
    (2, 64, 0, 12, 16, 128),        # 16-column tiles are 8 rows high
    (2, 81, 0, 16, 32, 128),        # C % 4 != 0: the persistent form declines the deferred norm
    (64, 64, 0, 64, 64, 256),       # enough items for the persistent form at level 1
    (64, 48, 0, 64, 64, 256),
    (64, 81, 0, 64, 64, 256),
    (64, 64, 0, 64, 16, 256),       # GELU-deferred at 16-column tiles: the one class level 1 keeps on 32x32x16
    (64, 20, 28, 64, 64, 224),
)
# route level -> per shape, per prenorm 0 | 1 | 2: (cf_conv2d_wino_form, cf_conv2d_wino_mfma), recorded from the build before wino_plan existed
_WINO_PLAN_RECORDED = {
    0: (((0, 0), (0, 0), (0, 0)),) * 15,
    1: (
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((8, 16), (8, 16), (8, 16)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 16), (2, 32), (2, 32)),
        ((8, 16), (8, 16), (8, 32)),
        ((8, 16), (0, 0), (0, 0)),
    ),
    2: (
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (2, 32), (2, 32)),
        ((2, 32), (0, 0), (0, 0)),
    ),
    4: (
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (0, 0), (0, 0)),
        ((4, 32), (4, 32), (4, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((4, 32), (4, 32), (4, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((0, 0), (0, 0), (0, 0)),
        ((0, 0), (0, 0), (0, 0)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (4, 32), (4, 32)),
        ((4, 32), (0, 0), (0, 0)),
    ),
    8: (
        ((8, 32), (8, 32), (8, 32)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 32), (0, 0), (0, 0)),
        ((8, 32), (8, 32), (8, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 32), (8, 32), (8, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 32), (8, 32), (8, 32)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 32), (0, 0), (0, 0)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 32), (0, 0), (0, 0)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 32), (0, 0), (0, 0)),
    ),
    16: (
        ((8, 16), (8, 16), (8, 16)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 16), (0, 0), (0, 0)),
        ((8, 16), (8, 16), (8, 16)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 16), (8, 16), (8, 16)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 16), (8, 16), (8, 16)),
        ((0, 0), (0, 0), (0, 0)),
        ((8, 16), (2, 32), (2, 32)),
        ((8, 16), (8, 16), (8, 16)),
        ((8, 32), (8, 32), (8, 32)),
        ((8, 16), (2, 32), (2, 32)),
        ((8, 16), (8, 16), (8, 16)),
        ((8, 16), (0, 0), (0, 0)),
    ),
}


def test_wino_probes_read_one_plan():
    """cf_conv2d_wino_ok, cf_conv2d_wino_form and cf_conv2d_wino_mfma read the one plan a launch executes (wino_plan, host code, no launch):
    ok is `form != 0`, the MFMA shape is 0 exactly where the form is, 16 only on the persistent form, and over shapes x route levels x
    deferred-norm classes both equal what the dispatch answered before the plan existed."""
    from cineflow import _lib, ops
    h = _lib.lib()
    prev = h.cf_conv_wino_enable(1)
    try:
        for level in (0, 1, 2, 4, 8, 16):
            h.cf_conv_wino_enable(level)
            for shape, recorded in zip(_WINO_PLAN_SHAPES, _WINO_PLAN_RECORDED[level]):
                for pre in (0, 1, 2):
                    form, mfma = ops.wino_form(*shape, prenorm=pre != 0), ops.wino_mfma(*shape, prenorm=pre)
                    what = (level, shape, pre)
                    assert ops.wino_ok(*shape, prenorm=pre != 0) == (form != 0), what
                    assert (mfma == 0) == (form == 0) and mfma in (0, 16, 32) and (mfma != 16 or form == 8), what
                    assert (form, mfma) == recorded[pre], what
    finally:
        h.cf_conv_wino_enable(prev)


def test_wino_plan_declines_a_norm_table_past_the_lds():
    """The one-tile form keeps the deferred norm's {mean, scale, shift} table of 3 * (C / 16) * 16 floats in LDS behind its two V buffers
    (2 * 6 patch rows * 5120 bytes at 32-column tiles, NTW 2).  C is the smallest multiple of 16 at which the sum passes 160 KiB: the probes
    accepted that shape (form 2) and the launch then failed with "LDS tile too large"; the plan declines it, and keeps the shape one chunk
    below.  The persistent form has no table and still takes both when forced."""
    from cineflow import _lib, ops
    C = next(c for c in range(16, 1 << 16, 16) if 2 * 6 * 5120 + 3 * (c // 16) * 16 * 4 > 160 * 1024)
    assert C == 8544
    h = _lib.lib()
    prev = h.cf_conv_wino_enable(1)
    try:
        for level in (1, 2):
            h.cf_conv_wino_enable(level)
            assert ops.wino_form(1, C, 0, 4, 32, 128, prenorm=True) == 0 and not ops.wino_ok(1, C, 0, 4, 32, 128, prenorm=True), level
            assert ops.wino_mfma(1, C, 0, 4, 32, 128, prenorm=1) == 0, level
            assert ops.wino_form(1, C - 16, 0, 4, 32, 128, prenorm=True) == 2, level
            assert ops.wino_form(1, C, 0, 4, 32, 128) == 2, level                  # no deferred norm, no table
        h.cf_conv_wino_enable(8)
        assert ops.wino_form(1, C, 0, 4, 32, 128, prenorm=True) == 8
    finally:
        h.cf_conv_wino_enable(prev)


CONV3D_PROBE_TABLE = os.path.join(ROOT, "tests", "golden", "conv3d_probe_table.json")


def _conv3d_probe_rows(lists, pointwise):
    import itertools
    keys = ("B", "C1", "D", "HW", "Cout", "sd", "s") if pointwise else ("B", "C1", "C2", "D", "HW", "Cout", "KD", "sd", "s")
    for v in itertools.product(*(lists[k] for k in keys)):
        r = dict(zip(keys, v))
        yield r if not pointwise else dict(r, C2=0, KD=1)


def _conv3d_probe_answers(h, lists, pointwise):
    bits = []
    for r in _conv3d_probe_rows(lists, pointwise):
        (H, W) = r["HW"]
        if pointwise:
            a = h.cf_conv3d_pw_f16s_ok(r["B"], r["C1"], r["D"], H, W, r["Cout"], r["sd"], r["s"])
        else:
            a = h.cf_conv3d_f16s_ok(r["B"], r["C1"], r["C2"], r["D"], H, W, r["Cout"], r["KD"], 3, r["sd"], r["s"])
        assert a in (0, 1), (r, a)
        bits.append(a)
    return bits


def _bits_to_hex(bits):
    return "%0*x" % ((len(bits) + 3) // 4, int("".join(map(str, bits)), 2))


def _hex_to_bits(s, n):
    return [int(c) for c in bin(int(s, 16))[2:].zfill(n)]


def test_conv3d_probe_table():
    """cf_conv3d_f16s_ok and cf_conv3d_pw_f16s_ok answer every row of a grid as the library did before the two files planned each launch
    once: tests/golden/conv3d_probe_table.json holds the grid's lists and, per probe, the recorded answers as one hex bit string in
    itertools.product order.  (CINEFLOW_WRITE_PROBE_TABLE=1 with CINEFLOW_LIB naming the library to record rewrites the file instead.)
    The grid reaches both answers often, every class of decline of the native probe -- one sample of 2 GiB or more; (a) no depth taps on a
    large map; (b) in-plane stride 2 at depth stride 1 on a large map; (c) few workgroups with a long K loop, or no geometry -- and
    B = 40 rows cut into sub-batches (40 is no multiple of most part counts), so the plan of a shorter last part is in the table.  The
    counts are the recorded library's."""
    import json
    from cineflow import _lib, ops
    h = _lib.lib()
    if os.environ.get("CINEFLOW_WRITE_PROBE_TABLE") == "1":
        lists = dict(B=[1, 2, 3, 40], C1=[1, 32, 40, 320], C2=[0, 16], D=[1, 2, 5, 20],
                     HW=[[4, 5], [8, 7], [12, 20], [32, 28], [128, 112], [256, 224], [512, 448]], Cout=[8, 32, 48, 320], KD=[1, 3], sd=[1, 2], s=[1, 2])
        table = dict(lists=lists, native=_bits_to_hex(_conv3d_probe_answers(h, lists, False)), pointwise=_bits_to_hex(_conv3d_probe_answers(h, lists, True)))
        with open(CONV3D_PROBE_TABLE, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    table = json.load(open(CONV3D_PROBE_TABLE))
    lists = table["lists"]
    for pointwise, name, n_rows, n_taken in ((False, "native", 28672, 22390), (True, "pointwise", 7168, 7080)):
        rows = list(_conv3d_probe_rows(lists, pointwise))
        want = _hex_to_bits(table[name], len(rows))
        assert len(rows) == n_rows and len(want) == n_rows and sum(want) == n_taken, (name, len(rows), sum(want))
        got = _conv3d_probe_answers(h, lists, pointwise)
        wrong = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
        assert not wrong, (name, len(wrong), wrong[:5])
        if pointwise:
            continue
        assert 10 * sum(want) >= n_rows and 10 * (n_rows - sum(want)) >= n_rows
        classes = {"2gib": 0, "a": 0, "b": 0, "c": 0}
        cut = cut_taken = 0
        for r, w in zip(rows, want):
            (H, W), pd = r["HW"], r["KD"] // 2
            Do, Ho, Wo = (r["D"] + 2 * pd - r["KD"]) // r["sd"] + 1, (H - 1) // r["s"] + 1, (W - 1) // r["s"] + 1
            per = 4 * max(max(r["C1"], r["C2"]) * r["D"] * H * W, r["Cout"] * Do * Ho * Wo)      # bytes of the largest tensor's sample
            if r["B"] == 40 and per < 2 ** 31 and r["B"] > (2 ** 31 - 1) // per:
                cut, cut_taken = cut + 1, cut_taken + w
            if not w:
                large = Do * Ho * Wo >= 65536
                cls = "2gib" if per >= 2 ** 31 else "a" if r["KD"] == 1 and large else "b" if r["s"] == 2 and r["sd"] == 1 and large else "c"
                classes[cls] += 1
        assert classes == {"2gib": 352, "a": 3024, "b": 736, "c": 2170}, classes
        assert (cut, cut_taken) == (1476, 781), (cut, cut_taken)
    assert ops.conv3d_f16s_ok(2, 32, 16, 5, 32, 28, 48, (3, 3, 3), (1, 1, 1)) and ops.conv3d_pw_f16s_ok(2, 32, 5, 32, 28, 48, (2, 2, 2))
    with ops.conv_terms(1):      # only the three-term product is built
        assert not ops.conv3d_f16s_ok(2, 32, 16, 5, 32, 28, 48, (3, 3, 3), (1, 1, 1)) and not ops.conv3d_pw_f16s_ok(2, 32, 5, 32, 28, 48, (2, 2, 2))


class _FakeTensor:
    """what the route decisions read of a tensor: its shape, its element count and an aligned address"""

    def __init__(self, *shape):
        self.shape = shape

    def numel(self):
        n = 1
        for v in self.shape:
            n *= v
        return n

    def data_ptr(self):
        return 0


def test_packed_conv_direct_takes_the_small_kernels_for_a_plain_call_only(monkeypatch):
    """convroute.PackedConv(direct=True) -- what nn.Conv2d builds -- sends a plain call of a 1 -> 32 3x3 stem to conv2d_small_cin and of a
    64 -> 2 3x3 head to conv2d_small_cout; any one of x2 / act / out / alpha != 1 / an overriding bias / set_conv_mode("f32") sends it back
    to the MFMA call.  res goes with small_cout only, stats_groups with small_cin only.  The same weights with direct=False (every other
    user of PackedConv) never take a direct kernel.  Host logic only: fake tensors, the ops launch functions replaced by recorders."""
    from cineflow import ops
    from cineflow.convroute import PackedConv
    calls = []
    for name in ("conv2d_small_cin", "conv2d_small_cout", "conv2d_f16s", "conv2d", "conv2d_wino"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)) or _n)
    monkeypatch.setattr(ops, "CONV_MODE", "f16s")
    g = torch.Generator().manual_seed(0)
    B, H, W = 2, 32, 48
    layers = {"stem": (torch.randn(32, 1, 3, 3, generator=g), torch.randn(32, generator=g)),
              "head": (torch.randn(2, 64, 3, 3, generator=g), torch.randn(2, generator=g))}
    direct_of = {"stem": "conv2d_small_cin", "head": "conv2d_small_cout"}
    for which, (w, b) in layers.items():
        cout, cin = w.shape[:2]
        conv = PackedConv(w, b, 1, (1, 1), wino=True, direct=True)
        plain = PackedConv(w, b, 1, (1, 1), wino=True)
        x, other = _FakeTensor(B, cin, H, W), _FakeTensor(B, cout, H, W)
        assert conv(x) == direct_of[which]
        name, a, k = calls[-1]
        assert a[0] is x and a[1] is w and a[2] is b, "the direct kernels read the checkpoint layout and the layer's own bias"
        back = [dict(x2=_FakeTensor(B, cin, H, W)), dict(act="relu"), dict(out=other), dict(alpha=0.5), dict(bias=None),
                dict(bias=torch.zeros(cout))]
        for kw in back:
            assert conv(x, **kw) == "conv2d_f16s", (which, kw)
        if which == "stem":
            assert conv(x, stats_groups=8) == "conv2d_small_cin" and calls[-1][1][3] == 8
            assert conv(x, stats_groups=128) == "conv2d_f16s"                        # more statistics groups than the direct kernel holds
            assert conv(x, res=other) == "conv2d_f16s"
        else:
            assert conv(x, res=other) == "conv2d_small_cout" and calls[-1][1][3] is other
            assert conv(x, stats_groups=2) == "conv2d_f16s"
        for kw in [{}] + back + [dict(res=other), dict(stats_groups=8)]:
            assert plain(x, **kw) == "conv2d_f16s", (which, kw)
        monkeypatch.setattr(ops, "CONV_MODE", "f32")
        assert conv(x) == "conv2d" and conv(x, stats_groups=8) == ("conv2d", None) and plain(x) == "conv2d"
        monkeypatch.setattr(ops, "CONV_MODE", "f16s")
    assert not [c for c in calls if c[0] == "conv2d_wino"]


def test_packed_conv3d_asks_native_then_pointwise_and_packs_once_per_split(monkeypatch):
    """convroute.PackedConv3d: the native kernel's probe is checked first and the pointwise one second, each for its own kernel shape (a
    (1|3, 3, 3) layer asks ops.conv3d_f16s_ok alone; a (1, 1, 1) layer asks ops.conv3d_pw_f16s_ok alone, and only without x2); None when the
    asked probe declines, when the shape is neither's, and under set_conv_mode("f32") (no probe is asked then).  The native packing is
    made once per distinct split key, the pointwise one once.  Host logic only: fake tensors, probes and launches replaced by recorders."""
    from cineflow import ops
    from cineflow.convroute import PackedConv3d
    log, answer = [], {"conv3d_f16s_ok": True, "conv3d_pw_f16s_ok": True}
    for name in answer:
        monkeypatch.setattr(ops, name, lambda *a, _n=name: log.append((_n, a)) or answer[_n])
    for name in ("conv3d_f16s", "conv3d_pw_f16s"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a, k)) or _n)
    monkeypatch.setattr(ops, "pack_conv3d_weight_f16s", lambda w, c1=None: log.append(("pack", c1)) or (("native", c1), 3))
    monkeypatch.setattr(ops, "pack_conv3d_pw_weight_f16s", lambda w: log.append(("pack_pw",)) or ("pw", 5))
    monkeypatch.setattr(ops, "CONV_MODE", "f16s")
    names = lambda: [e[0] for e in log]          # noqa: E731
    g = torch.Generator().manual_seed(0)
    bias = torch.randn(8, generator=g)

    conv = PackedConv3d(torch.randn(8, 32, 3, 3, 3, generator=g), bias, (1, 2, 2))
    x, x24, x8 = _FakeTensor(2, 32, 4, 8, 8), _FakeTensor(2, 24, 4, 8, 8), _FakeTensor(2, 8, 4, 8, 8)
    assert conv(x, None, 8) == "conv3d_f16s"
    assert log[0] == ("conv3d_f16s_ok", (2, 32, 0, 4, 8, 8, 8, (3, 3, 3), (1, 2, 2))) and names() == ["conv3d_f16s_ok", "pack", "conv3d_f16s"]
    name, a, k = log[-1]
    assert a[0] is x and a[1:] == (("native", None), 3, bias, 8, (3, 3, 3), (1, 2, 2)) and k == dict(x2=None, stats_groups=8)
    for x1, x2 in ((x24, x8), (x24, x8), (x, x8), (x, None)):          # split keys 24, 24, None (32 is whole chunks), None
        assert conv(x1, x2) == "conv3d_f16s"
    assert [e for e in log if e[0] == "pack"] == [("pack", None), ("pack", 24)]
    assert log[-1][1][1] == ("native", None) and "conv3d_pw_f16s_ok" not in names()
    del log[:]
    answer["conv3d_f16s_ok"] = False
    assert conv(x) is None and names() == ["conv3d_f16s_ok"]            # declined: the pointwise probe is not for this kernel shape
    monkeypatch.setattr(ops, "CONV_MODE", "f32")
    answer["conv3d_f16s_ok"] = True
    assert conv(x) is None and names() == ["conv3d_f16s_ok"]            # nothing more was asked
    monkeypatch.setattr(ops, "CONV_MODE", "f16s")

    del log[:]
    pw = PackedConv3d(torch.randn(8, 32, 1, 1, 1, generator=g), None, (2, 2, 2))
    assert pw(x, None, 8) == "conv3d_pw_f16s" and pw(x) == "conv3d_pw_f16s"
    assert names() == ["conv3d_pw_f16s_ok", "pack_pw", "conv3d_pw_f16s", "conv3d_pw_f16s_ok", "conv3d_pw_f16s"]
    assert log[0][1] == (2, 32, 4, 8, 8, 8, (2, 2, 2))
    assert log[2][1][1:] == ("pw", 5, None, 8, (2, 2, 2)) and log[2][2] == dict(stats_groups=8)
    del log[:]
    assert pw(x24, x8) is None and names() == []                        # cat[x, x2]: the pointwise kernel reads one input
    answer["conv3d_pw_f16s_ok"] = False
    assert pw(x) is None and names() == ["conv3d_pw_f16s_ok"]
    answer["conv3d_pw_f16s_ok"] = True
    monkeypatch.setattr(ops, "CONV_MODE", "f32")
    assert pw(x) is None and names() == ["conv3d_pw_f16s_ok"]
    monkeypatch.setattr(ops, "CONV_MODE", "f16s")
    del log[:]
    assert PackedConv3d(torch.randn(8, 32, 3, 1, 1, generator=g), None, (1, 1, 1))(x) is None and names() == []      # neither kernel's shape
