"""The bilinear-tap kernels held to their fp32 chain, bit for bit.  csrc/common.h gives csrc/warp.hip, the lookups of csrc/corr.hip and
sample_points_kernel one fully determined sequence of rounded operations (st_coord -> make_taps -> sample_taps), so every output element has
one right bit pattern: that of tests/_tap_chain.py, the numpy float32 restatement pinned in test_tap_chain_cpu.py.  There is no tolerance
in this file.  A row passes when the NaN positions of device and chain agree and every other element has the chain's bits (+0 is not -0);
the bits of a NaN itself are not compared (inf - inf is the negative quiet NaN on the CPU that runs numpy and the positive one on the
device).  test_gpu_ops.py and test_gpu_flow_op_shapes.py keep tying the same kernels to the reference's goldens and to oracle.ops at sizes
the numpy chain is too slow for.

Every output is a NaN-filled tensor (255 for labels) handed to the C ABI, so an element no kernel wrote fails the row.  A failing row prints
the count of differing elements, the first index, the chain's intermediates there (y, x, y0, x0, the four weights, the four taps, the result;
for memory_input those of the sampled plane `reg`, for the 3-D kernel the three positions and the eight corners) and the device value.  With pytest -s every row prints one line: elements, elements differing from the chain, and for context the same
output's worst distance from oracle.ops (differing pixels for labels): what the tolerance bars of the older tests absorb.

Resolving power on the device side: every row also asserts that the `contracted` variant of the chain (the tap sum as an FMA chain) differs
from the device output, and the label rows that `last_tie` (argmax taking >=) does: the row would have caught that kernel.  The label
kernels' class sums have no product feeding a sum (a select stands between), so `contracted` has no label form.  vecint with nsteps 0 is
the scaling alone and is held to the exact input instead.

entry point -> kernel -> rows.  Which kernel runs follows from the launch conditions in warp.hip (warp_v4: W % 4 == 0, every tensor on a
16-byte boundary, the label output on a 4-byte one) and in cf_corr_lookup (radius 4, levels <= 4, H W % 64 == 0); each row asserts the
condition its name states on the pointers it hands over.
  cf_warp_bilinear_2d    warp_bilinear_2d_v4_kernel<false>      test_warp_rows[v4 2x3x17x24, v4 2x1x17x24, v4 2x5x17x24]
                         warp_bilinear_2d_kernel                test_warp_rows[one-pixel 2x3x17x23, one-pixel 2x5x17x23,
                                                                one-pixel 2x3x17x24, views one float in (also bit-equal to the aligned run)]
  cf_vecint_2d           scale_kernel + warp_bilinear_2d_v4_kernel<true>              test_vecint_rows[3x20x32 ..., 1x256x256 nsteps 7]
                         scale_kernel + warp_bilinear_2d_kernel (addend)              test_vecint_rows[3x21x30 ...]
  cf_warp_labels_2d      warp_labels_2d_v4_kernel<4>            test_label_rows[v4<4> K=4 16x32]
                         warp_labels_2d_v4_kernel<0>            test_label_rows[v4<0> K=2, K=3, K=8 16x32]
                         warp_labels_2d_kernel                  test_label_rows[one-pixel K=4 16x30, K=3 16x30, K=4 16x32 output one byte in]
  cf_memory_input        memory_input_kernel                    test_memory_rows[3x20x32, 3x21x30]
  cf_sample_points_2d    sample_points_kernel                   test_sample_points_row
  cf_corr_lookup         corr_lookup_kernel                     test_lookup_rows[flat radius 3 ..., flat radius 4 ... (H W % 64 = 60)]
                         corr_lookup_tiled_kernel<16>           test_lookup_rows[tiled<16> ... 8x8 2 levels, ... 16x16 4 levels]
  cf_warp_trilinear_3d   warp_trilinear_3d_kernel               test_warp3d_rows

Non-finite flows (NaN, +inf, -inf) give NaN in the 2-D family (an invalid tap contributes 0 x NaN), 0 in the 3-D kernel (invalid corners are
skipped) and class 0 for labels; neither kernel form touches memory for them: the one-pixel kernels clamp the index to [-2, size + 1] and
issue no load for an invalid tap, the four-pixel kernels send an invalid tap to offset 0x80000000 of a buffer resource sized to the tensor,
which returns 0.  Measured figures: profiles/tap_chain_table.md.
"""
import numpy as np
import pytest
import torch

import _tap_chain as TC

pytestmark = pytest.mark.gpu

NAN = float("nan")
T = torch.from_numpy


def call(name, *args):
    from cineflow._lib import check, lib
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    check(getattr(lib(), name)(*a, torch.cuda.current_stream().cuda_stream), name)


def filled(dev, *shape, dtype=torch.float32, lead=None):
    """the stale-memory guard: NaN (255 for labels) until a kernel writes; lead: as a contiguous view `lead` elements into a fenced buffer"""
    fill = 255 if dtype == torch.uint8 else NAN
    if lead is None:
        t = torch.full(shape, fill, dtype=dtype, device=dev)
        assert t.data_ptr() % 16 == 0
        return t, None
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), fill, dtype=dtype, device=dev)
    return buf[lead:lead + n].view(shape), buf


def put(x, dev, lead=None):
    """x (numpy) on the device; lead: a contiguous view `lead` elements into a buffer fenced by NaNs / 255s"""
    x = T(np.ascontiguousarray(x))
    if lead is None:
        xd = x.to(dev)
        assert xd.data_ptr() % 16 == 0
        return xd
    view, _ = filled(dev, *x.shape, dtype=x.dtype, lead=lead)
    view.copy_(x.to(dev))
    assert view.is_contiguous() and view.data_ptr() % 16 == (lead * x.element_size()) % 16
    return view


def fences_hold(view, buf, lead):
    edge = torch.cat([buf[:lead], buf[lead + view.numel():]])
    return bool((edge == 255).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(edge).all())


def aligned16(*tensors):
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def mismatches(got, want):
    """boolean map of the elements where `got` is not the chain's `want`: NaN against non-NaN, or different bits (module docstring)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.uint8:
        return got != want
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (got.view(np.int32) != want.view(np.int32)))


def hold(tag, got, want, locate=None, oracle=None):
    """assert that the device output has the chain's bits in every element; prints the row's line"""
    got = got.detach().cpu().contiguous().numpy() if isinstance(got, torch.Tensor) else got
    bad = mismatches(got, want)
    n = int(bad.sum())
    line = "  %-64s %8d elements, %d differ from the chain" % (tag, got.size, n)
    if oracle is not None:
        oracle = np.asarray(oracle.numpy() if isinstance(oracle, torch.Tensor) else oracle)
        assert oracle.shape == got.shape
        if got.dtype == np.uint8:
            line += "; %d pixels differ from oracle.ops" % int((got.astype(np.int64) != oracle.astype(np.int64)).sum())
        else:
            both = np.isfinite(got) & np.isfinite(oracle)
            line += "; worst distance from oracle.ops %.3e" % float(np.abs(got[both].astype(np.float64) - oracle[both].astype(np.float64)).max())
    print(line)
    if n:
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        where = locate(first) if locate is not None else "(no intermediates for this row)"
        print("  %s: FIRST of %d differing elements at %r\n    chain: %s\n    chain value %r, device value %r" % (
            tag, n, first, where, want[first].item(), got[first].item()))
    assert n == 0, "%s: %d of %d elements differ from the chain, first at %r: chain %r, device %r" % (
        tag, n, got.size, first, want[first].item(), got[first].item())
    return got


def resolves(tag, got, variant_out, what="contracted"):
    n = int(mismatches(got, variant_out).sum())
    print("      the `%s` variant differs from the device in %d elements" % (what, n))
    assert n > 0, "%s: the `%s` variant equals the device output: this row could not have caught that kernel" % (tag, what)
    return n


def image_locator(detail, W):
    """index (b, c, i, j) of an image-shaped output -> the chain's intermediates there (detail arrays are [B, C, H W])"""
    return lambda idx: TC.explain(detail, (idx[0], min(idx[1], detail["result"].shape[1] - 1), idx[2] * W + idx[3]))


# ===================================================================================================== cf_warp_bilinear_2d
def c_warp(dev, flow, src, lead):
    B, C, H, W = src.shape
    fd, sd = put(flow, dev, lead), put(src, dev, lead)
    out, buf = filled(dev, B, C, H, W, lead=lead)
    call("cf_warp_bilinear_2d", fd, sd, out, B, C, H, W)
    torch.cuda.synchronize()
    assert buf is None or fences_hold(out, buf, lead), "fence overwritten"
    return out, (W % 4 == 0 and aligned16(fd, sd, out))


@pytest.mark.parametrize("name", list(TC.WARP_ROWS))
def test_warp_rows(dev, name):
    from oracle import ops as OO
    B, C, H, W, view = TC.WARP_ROWS[name]
    flows, src = TC.warp_row_inputs(name)
    print()
    for fname, flow in flows.items():
        tag = "warp %s, %s" % (name, fname)
        out, v4 = c_warp(dev, flow, src, 1 if view else None)
        assert v4 == name.startswith("v4"), "%s: launch condition of the four-pixel kernel is %s" % (tag, v4)
        want, det = TC.warp2d(flow, src, detail=True)
        got = hold(tag, out, want, image_locator(det, W), OO.warp_bilinear(T(flow).clone(), T(src)))
        resolves(tag, got, TC.warp2d(flow, src, variant="contracted"))
        if view:                                         # the one-pixel kernel on a W % 4 == 0 map: the aligned run's bits (NaNs included)
            base, base_v4 = c_warp(dev, flow, src, None)
            assert base_v4 and torch.equal(out.contiguous().view(torch.int32), base.view(torch.int32)), "%s: differs from the aligned run" % tag
        if fname == "nonfinite":
            for _, i, j in TC.nonfinite_pixels(H, W):
                assert np.isnan(got[0, :, i, j]).all(), (tag, i, j)
            assert int(np.isnan(got).sum()) == 6 * C
        if fname == "far":
            assert not np.isnan(got).any()
            for k in range(len(TC.FAR)):
                assert (got[0, :, [1, 3, 5, 7, 9], [2 + k, 2 + k, 2 + k, 2 + k, 2 + 2 * k]] == 0).all(), (tag, k)


# ===================================================================================================== cf_vecint_2d
@pytest.mark.parametrize("name", list(TC.VECINT_ROWS))
def test_vecint_rows(dev, name):
    from oracle import ops as OO
    B, H, W, nsteps, nan_at = TC.VECINT_ROWS[name]
    vec, _ = TC.vecint_row_inputs(name)
    vd = put(vec, dev)
    (out, _), (tmp, _) = filled(dev, B, 2, H, W), filled(dev, B, 2, H, W)
    call("cf_vecint_2d", vd, out, tmp, B, H, W, nsteps)
    torch.cuda.synchronize()
    print()
    tag = "vecint " + name
    want, det = TC.vecint2d(vec, nsteps, detail=True)
    oracle = None if nan_at is not None else OO.vecint(T(vec).clone(), nsteps)
    got = hold(tag, out, want, None if det is None else image_locator(det, W), oracle)
    if nsteps == 0:
        assert np.array_equal(got.view(np.int32), vec.view(np.int32)), "nsteps 0: scaling by 1.0f is the input"
    else:
        resolves(tag, got, TC.vecint2d(vec, nsteps, variant="contracted"))
    if nan_at is not None:
        nan = np.isnan(got)
        print("    NaN spread from one pixel over %d steps: %d elements" % (nsteps, int(nan.sum())))
        assert nan[nan_at] and np.array_equal(nan, np.isnan(want))


# ===================================================================================================== cf_warp_labels_2d
@pytest.mark.parametrize("name", list(TC.LABEL_ROWS))
def test_label_rows(dev, name):
    from oracle import ops as OO
    Tn, B, K, H, W, lead = TC.LABEL_ROWS[name]
    flow, random, checker = TC.label_row_inputs(name)
    fd = put(flow, dev)
    print()
    for lname, lab in (("random labels", random), ("checkerboard", checker)):
        tag = "labels %s, %s" % (name, lname)
        out, buf = filled(dev, Tn, B, H, W, dtype=torch.uint8, lead=lead or None)
        call("cf_warp_labels_2d", fd, put(lab, dev), out, Tn, B, K, H, W)
        torch.cuda.synchronize()
        assert buf is None or (out.data_ptr() % 4 == 1 and fences_hold(out, buf, lead)), "fence overwritten"
        v4 = W % 4 == 0 and aligned16(fd) and out.data_ptr() % 4 == 0
        assert v4 == name.startswith("v4") and ("<4>" in name) == (v4 and K == 4), tag
        want, det = TC.warp_labels2d(flow, lab, K, detail=True)
        finite = np.isfinite(flow).all(2) & (np.abs(flow) < 1e5).all(2)                   # the oracle (ATen) is compared where the flow is tame
        oracle = OO.warp_labels(T(np.where(np.isfinite(flow) & (np.abs(flow) < 1e5), flow, np.float32(1e4))), T(lab)[:, None].float(), K)[:, :, 0].numpy()
        got = hold(tag, out, want, lambda idx: TC.explain(det, (idx[0] * B + idx[1], 0, idx[2] * W + idx[3])),
                   np.where(finite, oracle, want).astype(np.uint8))
        resolves(tag, got, TC.warp_labels2d(flow, lab, K, variant="last_tie"), "last_tie")
        assert int(got.max()) <= K - 1
        for _, i, j in TC.nonfinite_pixels(H, W):                                         # frame 0, sample 0: nothing sampled -> class 0
            assert got[0, 0, i, j] == 0, (tag, i, j)
        assert (got[0, 1, 11, 3:3 + len(TC.FAR)] == 0).all() and (got[0, 1, 12, 3:3 + len(TC.FAR)] == 0).all(), tag


# ===================================================================================================== cf_memory_input
@pytest.mark.parametrize("name", list(TC.MEMORY_ROWS))
def test_memory_rows(dev, name):
    from oracle import ops as OO
    B, H, W = TC.MEMORY_ROWS[name]
    x0, xt, flows = TC.memory_row_inputs(name)
    x0d, xtd = put(x0, dev), put(xt, dev)
    print()
    for fname, cum in flows.items():
        tag = "memory_input %s, %s" % (name, fname)
        out, _ = filled(dev, B, 6, H, W)
        call("cf_memory_input", x0d, xtd, put(cum, dev), out, B, H, W)
        torch.cuda.synchronize()
        want, det = TC.memory_input(x0, xt, cum, detail=True)
        reg = OO.warp_bilinear(T(cum).clone(), T(xt))
        got = hold(tag, out, want, lambda idx: "reg = warp(cum, xt): " + image_locator(det, W)(idx),
                   torch.cat([T(x0), T(xt), T(cum), T(x0) - reg, reg], 1))
        copies = np.concatenate([x0, xt, cum], axis=1)
        assert np.array_equal(got[:, :4].view(np.int32), copies.view(np.int32)), "%s: planes 0-3 are copies" % tag
        resolves(tag, got, TC.memory_input(x0, xt, cum, variant="contracted"))
        if fname == "nonfinite":
            assert int(np.isnan(got[:, 4:]).sum()) == 12 and all(np.isnan(got[0, 4:, i, j]).all() for _, i, j in TC.nonfinite_pixels(H, W))


# ===================================================================================================== cf_sample_points_2d
def test_sample_points_row(dev):
    field, pts = TC.sample_points_inputs()
    B, C, H, W = field.shape
    P = pts.shape[2]
    assert (B, C, H, W, P) == (2, 3, 9, 13, 257)
    out, _ = filled(dev, B, C, P)
    call("cf_sample_points_2d", put(field, dev), put(pts, dev), out, B, C, H, W, P)
    torch.cuda.synchronize()
    print()
    want, det = TC.sample_points(field, pts, detail=True)
    import torch.nn.functional as F
    tame = np.where(np.isfinite(pts) & (np.abs(pts) < 1e5), pts, np.float32(1e4))
    grid = torch.stack([2 * (T(tame[:, 0]) / (W - 1) - 0.5), 2 * (T(tame[:, 1]) / (H - 1) - 0.5)], -1)[:, None]
    got = hold("sample_points 2x3x9x13, P = 257", out, want, lambda idx: TC.explain(det, idx), F.grid_sample(T(field), grid, align_corners=True)[:, :, 0])
    resolves("sample_points", got, TC.sample_points(field, pts, variant="contracted"))
    bad = ~np.isfinite(pts).all(1)
    assert np.array_equal(np.isnan(got), np.broadcast_to(bad[:, None], got.shape)) and int(bad.sum()) == 6


# ===================================================================================================== cf_corr_lookup
@pytest.mark.parametrize("name", list(TC.LOOKUP_ROWS))
def test_lookup_rows(dev, name):
    """the chain applied to the pyramid the kernel reads: the device's own, downloaded, as the lookup rows of test_gpu_flow_op_shapes.py
    apply the oracle (the 6 x 10 map, which cf_corr_pyramid does not take, looks up an uploaded one as test_second_trip_flat_lookup does)"""
    from cineflow import ops
    from oracle import ops as OO
    B, C, H, W, levels, radius, tiled = TC.LOOKUP_ROWS[name]
    f1, f2, coords = TC.lookup_row_inputs(name)
    if (H * W) % 64 == 0:
        pyr = ops.corr_pyramid(put(f1, dev), put(f2, dev), levels)
    else:                                                # cf_corr_pyramid takes H W % 64 == 0 only: the fp64 pyramid rounded to fp32, uploaded
        from _kernel_refs import allpairs_pyramid
        pyr = torch.cat([p.float().reshape(-1) for p in allpairs_pyramid(T(f1), T(f2), levels)]).to(dev)
    assert pyr.numel() == ops.pyramid_numel(B, H, W, levels)
    flat, lv, off = pyr.cpu().numpy(), [], 0
    for l in range(levels):
        n = B * H * W * (H >> l) * (W >> l)
        lv.append(flat[off:off + n].reshape(B, H * W, H >> l, W >> l))
        off += n
    assert off == flat.size
    D = 2 * radius + 1
    out, _ = filled(dev, B, levels * D * D, H, W)
    call("cf_corr_lookup", pyr, put(coords, dev), out, B, H, W, levels, radius)
    torch.cuda.synchronize()
    print()
    want, dets = TC.corr_lookup(lv, coords, radius, detail=True)

    def locate(idx):
        b, ch, y, x = idx
        return "level %d: " % (ch // (D * D)) + TC.explain(dets[ch // (D * D)], (b * H * W + y * W + x, 0, ch % (D * D)))

    tag = "lookup " + name
    got = hold(tag, out, want, locate, OO.corr_lookup([T(np.ascontiguousarray(p)) for p in lv], T(coords), radius))
    resolves(tag, got, TC.corr_lookup(lv, coords, radius, variant="contracted"))


# ===================================================================================================== cf_warp_trilinear_3d
def test_warp3d_rows(dev):
    from oracle import ops as OO
    flows, src = TC.warp3d_inputs()
    B, C, D, H, W = src.shape
    assert (B, C, D, H, W) == (2, 2, 5, 9, 7)
    sd = put(src, dev)
    print()
    for fname, flow in flows.items():
        tag = "warp 3-D 2x2x5x9x7, " + fname
        out, _ = filled(dev, B, C, D, H, W)
        call("cf_warp_trilinear_3d", put(flow, dev), sd, out, B, C, D, H, W)
        torch.cuda.synchronize()
        tame = np.where(np.isfinite(flow) & (np.abs(flow) < 1e5), flow, np.float32(1e4))
        want, det = TC.warp3d(flow, src, detail=True)
        got = hold(tag, out, want, lambda idx: TC.explain3d(det, (idx[0], idx[1], (idx[2] * H + idx[3]) * W + idx[4])),
                   OO.warp_bilinear(T(tame).clone(), T(src)))
        resolves(tag, got, TC.warp3d(flow, src, variant="contracted"))
        if fname == "nonfinite":
            assert not np.isnan(got).any()
            for z, y, x in TC.nonfinite_voxels():
                assert (got[0, :, z, y, x].view(np.int32) == 0).all(), (tag, z, y, x)     # +0: no corner sampled
