"""Shape tables for the operators of the flow network (csrc/warp.hip, csrc/allpairs.hip, the RAFT half of csrc/corr.hip) and the flat
plumbing kernels of csrc/elementwise.hip, at the shapes the older tests of test_gpu_ops.py leave out: launches whose grid-stride loop takes a
second trip, RAFT maps with H != W, both members of every one-pixel / four-pixel kernel pair per entry point, the minimum legal sizes, and
contiguous views that are not 16-byte aligned.

Second trips.  flat_grid caps a launch at 4096 workgroups of 256 threads: a one-item-per-thread kernel loops above 1,048,576 items, a
four-pixel kernel above 4,194,304 pixels.  The rows below use
    65 x 256 x 256 = 4,259,840 pixels  (four-pixel kernels; warp_labels as T, B = 5, 13: `tb % B` wraps in the second trip too)
    17 x 250 x 250 = 1,062,500 pixels  (one-pixel kernels, W % 4 == 2; warp_labels as T, B = 3, 6 = 1,125,000; the 3-D pair as 1 x 17 x 250 x 250)
and every output is a NaN-filled (255-filled for labels) tensor handed to the C ABI, so a trip that never ran shows as NaN rather than as
a stale correct value.  Each such row prints its worst figure over the whole output and over the items past the first trip.

References and bars.  Warp family: oracle.ops (pinned to the reference by test_oracle_golden.py), 2e-6 (2e-5 with far flows), the Jacobian
array_equal with numpy, labels at most 2 tie pixels (the bar of test_warp_labels; measured below: 0 at every size), vecint 1e-5 on fields
drawn at the golden fixtures' amplitude (their standard deviation, 3.0).  Pyramids: the fp64 restatement _kernel_refs.allpairs_pyramid
(pinned in test_kernel_refs_cpu.py), 3e-5 on unit-normal features, and levels 1.. bit-equal to pooling the stored previous level.  Lookups:
oracle.ops.corr_lookup on the device's own (downloaded) pyramid, 3e-5.  Convex upsampling 1e-5.  Copies and one-operation elementwise
kernels: 0.  Two bars are this module's own: gru_blend is three fp32 operations that the compiler may contract, judged against fp64 within
2^-22 x (|h| + |cand|) per element (three roundings of terms bounded by |h| + |cand|, one spare); tta_accumulate keeps the 1e-6 of
test_tta_and_tiles at logits and accumulators of the same scale.

entry point -> kernel -> test
  cf_warp_bilinear_2d     warp_bilinear_2d_v4_kernel<false> / warp_bilinear_2d_kernel      test_second_trip_2d[warp-*], test_small_2d, test_misaligned_views
  cf_vecint_2d            scale_kernel + warp_bilinear_2d_v4_kernel<true> / warp_bilinear_2d_kernel (addend)
                                                                                           test_second_trip_2d[vecint-*], test_vecint_tails, test_small_2d, test_misaligned_views
  cf_warp_labels_2d       warp_labels_2d_v4_kernel<4>, <0> / warp_labels_2d_kernel         test_second_trip_2d[labels-*], test_small_2d, test_misaligned_views
  cf_memory_input         memory_input_kernel                                              test_second_trip_2d[memory-flat], test_memory_input_widths, test_small_2d
  cf_jacobian_det_2d      jacobian_det_2d_v4_kernel / jacobian_det_2d_kernel               test_second_trip_2d[jacobian-*], test_small_2d, test_misaligned_views
  cf_warp_trilinear_3d    warp_trilinear_3d_kernel                                         test_second_trip_3d, test_small_3d, test_warp_3d_edge_cases
  cf_jacobian_det_3d      jacobian_det_3d_kernel                                           test_second_trip_3d, test_small_3d
  cf_corr_pyramid         allpairs_pyramid_kernel (W == 32, H % 16 == 0, C % 16 == 0, 4 levels, grid % 8 == 0)
                          / the fp32 GEMM + avgpool2x2_kernel                              test_raft_maps, test_second_trip_generic_pyramid
  cf_corr_lookup          corr_lookup_tiled_kernel<16> / corr_lookup_kernel                test_raft_maps, test_tiled_lookup_coarsest_2x2, test_tiled_lookup_equals_flat_kernel,
                                                                                           test_second_trip_flat_lookup
  cf_convex_upsample      convex_upsample_kernel (C = 4)                                   test_second_trip_convex_upsample
                          convex_upsample_rows_kernel<1>, <2> (one workgroup per map row: no grid-stride loop) stay with
                          test_gpu_ops.py::test_convex_upsample and ::test_convex_upsample_single_channel
  cf_corr_volume          not a RAFT operator: all three of its kernels have their table in test_gpu_corr_volume_routes.py
  cf_gru_reset_mul, cf_gru_blend, cf_binary, cf_copy_channels, cf_crop2d, cf_pad2d, cf_flip2d, cf_tta_accumulate, cf_tile_accumulate,
  cf_tile_finalize, cf_argmax_channels, cf_coords_grid, cf_count_out_of_range -> the kernel of the same name -> test_second_trip_elementwise_*

Measured on the MI355X (pytest -s prints one line per row: worst figure, bar, ratio):
  second trips, warp family: warp 4.8e-7 (2.4e-7 past the first trip) at both sizes; memory_input 4.8e-7; labels 0 differing pixels of
      4,259,840 and of 1,125,000; both Jacobians and the 3-D warp identical to numpy / ATen (0)
  vecint, nsteps 2, at the 1e-5 bar: 3.2e-6 at 66600 x 8 x 8 (4,262,400 px), 2.4e-6 at 22000 x 8 x 6 (1,056,000 px); 3 x 21 x 30 and
      3 x 20 x 32: <= 3.6e-6 for nsteps 0, 1, 2, 7.  At the full map width the 1e-5 of the 32- and 40-pixel fixtures does not hold between
      two fp32 implementations that associate the tap sum differently, as the kernel and ATen do (see VECINT_BIG; against its own fp32 chain
      the kernel is bit-equal there, nsteps 7 included: test_gpu_tap_chains.py); those rows take four times the oracle's own fp32-against-fp64 error, measured in the row
      on the CPU: oracle 1.69e-4 -> bar 6.8e-4, kernel 6.3e-5 at 65 x 256 x 256; oracle 1.64e-4 -> bar 6.6e-4, kernel 6.2e-5 at 17 x 250 x 250
  flat lookup 3.6e-7; convex upsample (C = 4) 5.7e-6; generic pyramid 32 x 64 1.7e-6; gru_blend 0.47 of its bound; tta_accumulate 2.7e-7;
      every copy, binary, crop / pad / flip, coords_grid, tile and argmax row 0; cf_count_out_of_range exact in all four launches
  RAFT maps: every level of all eight rows <= 1.2e-6 (bar 3e-5) and the pool of the stored level before it; every tiled lookup <= 4.8e-7;
      tiled == flat kernel on all 497,664 + 663,552 values
  small sizes and misaligned views: warp <= 2.4e-7, vecint <= 6.0e-6, labels 0, Jacobians 0; one-pixel kernels bit-equal to the four-pixel ones

One finding.  At C = 32 the fused kernel's level 1 was not the pool of its stored level 0 (rows fused 2 x 32 x 16 x 32 and 2 x 32 x 48 x 32;
C = 16 and the C = 256 of test_gpu_ops.py have a power-of-two 1 / sqrt(C), where it cannot show): the compiler contracted acc * scale into
the first sums of each 2 x 2 window.  allpairs.hip is built without contraction; both rows hold.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _kernel_refs import allpairs_pyramid, ratio_line

pytestmark = pytest.mark.gpu

TRIP1 = 4096 * 256                      # items of the first trip of a one-item-per-thread launch
NAN = float("nan")


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rand_labels(*shape, K, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * K).to(torch.uint8)


def filled(dev, *shape, dtype=torch.float32):
    """the stale-memory guard: NaN (255 for labels) until a kernel writes"""
    return torch.full(shape, 255 if dtype == torch.uint8 else NAN, dtype=dtype, device=dev)


def call(name, *args):
    from cineflow._lib import check, lib
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    check(getattr(lib(), name)(*a, torch.cuda.current_stream().cuda_stream), name)


def row(tag, got, want, bar, first=None, channels=False):
    """max|got - want| <= bar over the whole output; with `first`, the same figure over the items (pixels; over the channel axis 1 when
    `channels`) from index `first` on is printed too"""
    got = got.detach().cpu()
    want = torch.as_tensor(want)
    assert tuple(got.shape) == tuple(want.shape), (tag, got.shape, want.shape)
    d = (got.double() - want.double()).abs()
    worst = float(d.max())
    ratio_line(tag, worst, bar)
    if first is not None:
        per_item = d.flatten(2).amax(1).reshape(-1) if channels else d.reshape(-1)
        assert per_item.numel() > first, (tag, per_item.numel(), first)
        ratio_line("    %d items past %d" % (per_item.numel() - first, first), float(per_item[first:].max()), bar)
    assert worst <= bar, "%s: max|diff| %.3e > %.1e (NaN: an element no kernel wrote)" % (tag, worst, bar)      # NaN <= bar is False


def label_row(tag, got, want, first=None):
    got, want = got.cpu().long(), want.long()
    assert got.shape == want.shape
    bad = got != want
    ratio_line(tag + ": differing pixels", float(bad.sum()), 2)
    if first is not None:
        assert bad.numel() > first
        ratio_line("    %d items past %d" % (bad.numel() - first, first), float(bad.reshape(-1)[first:].sum()), 2)
    assert int((got == 255).sum()) == 0, "%s: %d pixels no kernel wrote" % (tag, int((got == 255).sum()))
    assert int(bad.sum()) <= 2, "%s: %d pixels differ (ties at class borders only: <= 2)" % (tag, int(bad.sum()))


def jacobian_ref(disp):
    from oracle import ops as OO
    perm = (1, 2, 0) if disp.dim() == 4 else (1, 2, 3, 0)
    return np.stack([OO.jacobian_determinant(disp[b].permute(*perm).numpy().astype(np.float64)) for b in range(disp.shape[0])])


def jacobian_row(tag, got, disp, first=None):
    got, want = got.cpu().numpy(), jacobian_ref(disp)
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    ratio_line(tag + ": values differing from numpy", float(bad.sum()), 0)
    if first is not None:
        ratio_line("    %d items past %d" % (bad.size - first, first), float(bad.reshape(-1)[first:].sum()), 0)
    assert np.array_equal(got, want), "%s: %d values differ, max|diff| %.3e" % (tag, bad.sum(), np.nanmax(np.abs(got - want)))


@pytest.fixture(scope="module")
def vec_amp(golden):
    """the amplitude of the golden fixtures' vecint fields (3.0 x unit normal)"""
    a = float(np.std(golden("warp_40x24")["flow"]))
    assert 2.5 < a < 3.5, a
    return a


# the C ABI on explicit outputs ------------------------------------------------------------------------------------------------
def c_warp(flow, src, out=None):
    B, C, H, W = src.shape
    out = filled(src.device, B, C, H, W) if out is None else out
    call("cf_warp_bilinear_2d", flow, src, out, B, C, H, W)
    return out


def c_vecint(vec, nsteps, out=None, tmp=None):
    B, _, H, W = vec.shape
    out = filled(vec.device, B, 2, H, W) if out is None else out
    tmp = filled(vec.device, B, 2, H, W) if tmp is None else tmp
    call("cf_vecint_2d", vec, out, tmp, B, H, W, nsteps)
    return out


def c_labels(flow, lab, K, out=None):
    T, B, _, H, W = flow.shape
    out = filled(flow.device, T, B, H, W, dtype=torch.uint8) if out is None else out
    call("cf_warp_labels_2d", flow, lab, out, T, B, K, H, W)
    return out


def c_memory(x0, xt, cum):
    B, _, H, W = x0.shape
    out = filled(x0.device, B, 6, H, W)
    call("cf_memory_input", x0, xt, cum, out, B, H, W)
    return out


def c_jacobian(disp, out=None):
    B, _, H, W = disp.shape
    out = filled(disp.device, B, H, W, dtype=torch.float64) if out is None else out
    call("cf_jacobian_det_2d", disp, out, B, H, W)
    return out


def c_warp3(flow, src):
    B, C, D, H, W = src.shape
    out = filled(src.device, B, C, D, H, W)
    call("cf_warp_trilinear_3d", flow, src, out, B, C, D, H, W)
    return out


def c_jacobian3(disp):
    B, _, D, H, W = disp.shape
    out = filled(disp.device, B, D, H, W, dtype=torch.float64)
    call("cf_jacobian_det_3d", disp, out, B, D, H, W)
    return out


def memory_ref(x0, xt, cum):
    from oracle import ops as OO
    reg = OO.warp_bilinear(cum.clone(), xt)
    return torch.cat([x0, xt, cum, x0 - reg, reg], 1)


# ================================================================================================= rows 1 + 2: second grid trips, warp family
BIG = {"v4": (65, 256, 256, 4 * TRIP1), "flat": (17, 250, 250, TRIP1)}      # frames, H, W, pixels of the first trip
# vecint feeds one warp's output to the next as a displacement: two fp32 implementations whose first step differs by one ulp (the kernel's
# chain and ATen's vectorised sampler associate differently; the kernel is bit-equal to its own chain, test_gpu_tap_chains.py) differ by one
# ulp of (j + v) in the second step's sampling position -- 3.1e-5 px at j >= 128 -- times the field's slope, which is |v| itself where the
# sample leaves the image (zero padding).  The 1e-5 of the 32- and 40-pixel golden fixtures therefore holds on maps of that size, not at 256
# (module docstring: measured 5.7e-5 and 6.3e-5 there, and the same from the oracle against itself).  The second-trip rows of vecint reach
# their pixel count with many small frames instead:
VECINT_BIG = {"v4": (66600, 8, 8), "flat": (22000, 8, 6)}                    # 4,262,400 and 1,056,000 pixels


@pytest.mark.parametrize("entry,kind", [("warp", "v4"), ("vecint", "v4"), ("labels", "v4"), ("jacobian", "v4"),
                                        ("warp", "flat"), ("vecint", "flat"), ("labels", "flat"), ("jacobian", "flat"), ("memory", "flat")])
def test_second_trip_2d(dev, vec_amp, entry, kind):
    from oracle import ops as OO
    n, H, W, first = BIG[kind]
    assert n * H * W > first and (W % 4 == 0) == (kind == "v4")
    seed = {"warp": 1000, "vecint": 1010, "labels": 1020, "jacobian": 1030, "memory": 1040}[entry] + 5 * (kind == "v4")
    tag = "%s %d x %d x %d (%d px > %d)" % (entry, n, H, W, n * H * W, first)
    print()
    if entry == "warp":
        flow, src = 3.0 * randn(n, 2, H, W, seed=seed), randn(n, 1, H, W, seed=seed + 1)
        row(tag, c_warp(flow.to(dev), src.to(dev)), OO.warp_bilinear(flow.clone(), src), 2e-6, first)
    elif entry == "vecint":
        n, H, W = VECINT_BIG[kind]
        assert n * H * W > first and (W % 4 == 0) == (kind == "v4")
        vec = vec_amp * randn(n, 2, H, W, seed=seed)
        row("vecint %d x %d x %d (%d px > %d), nsteps 2" % (n, H, W, n * H * W, first), c_vecint(vec.to(dev), 2), OO.vecint(vec.clone(), 2), 1e-5, first,
            channels=True)
        # and at the full map width (columns j >= 128 of the addend path), where the bar is four times the oracle's own fp32 error against
        # the same recursion in fp64, measured here on the CPU
        n, H, W, first = BIG[kind]
        vec = vec_amp * randn(n, 2, H, W, seed=seed + 2)
        ref = OO.vecint(vec.clone(), 2)
        own = float((ref.double() - OO.vecint(vec.double(), 2)).abs().max())
        print("  oracle fp32 against fp64 at %d x %d x %d: %.3e" % (n, H, W, own))
        assert 2e-5 < own < 1e-3, own
        row("vecint %d x %d x %d (%d px > %d), nsteps 2, bar 4 x %.2e" % (n, H, W, n * H * W, first, own), c_vecint(vec.to(dev), 2), ref, 4 * own, first,
            channels=True)
    elif entry == "labels":
        T, B = (5, 13) if kind == "v4" else (3, 6)
        assert T * B * H * W > first
        flow, lab = 3.0 * randn(T, B, 2, H, W, seed=seed), rand_labels(B, H, W, K=4, seed=seed + 1)
        assert int(lab.max()) == 3
        label_row("labels T, B = %d, %d at %d x %d (%d px > %d)" % (T, B, H, W, T * B * H * W, first), c_labels(flow.to(dev), lab.to(dev), 4),
                  OO.warp_labels(flow, lab[:, None].float())[:, :, 0], first)
    elif entry == "jacobian":
        disp = 3.0 * randn(n, 2, H, W, seed=seed)
        jacobian_row(tag, c_jacobian(disp.to(dev)), disp, first)
    else:
        x0, xt, cum = randn(n, 1, H, W, seed=seed), randn(n, 1, H, W, seed=seed + 1), 3.0 * randn(n, 2, H, W, seed=seed + 2)
        row(tag, c_memory(x0.to(dev), xt.to(dev), cum.to(dev)), memory_ref(x0, xt, cum), 2e-6, first, channels=True)


def test_second_trip_3d(dev):
    from oracle import ops as OO
    B, D, H, W = 1, 17, 250, 250
    assert B * D * H * W > TRIP1
    print()
    flow, src = 2.0 * randn(B, 3, D, H, W, seed=1101), randn(B, 1, D, H, W, seed=1102)
    row("warp 3-D %d x %d x %d x %d (%d > %d)" % (B, D, H, W, B * D * H * W, TRIP1), c_warp3(flow.to(dev), src.to(dev)),
        OO.warp_bilinear(flow.clone(), src), 2e-6, TRIP1)
    disp = 2.0 * randn(B, 3, D, H, W, seed=1103)
    jacobian_row("jacobian 3-D %d x %d x %d x %d" % (B, D, H, W), c_jacobian3(disp.to(dev)), disp, TRIP1)


# ================================================================================================= row 2: second trips, RAFT and plumbing
def test_second_trip_flat_lookup(dev):
    """corr_lookup_kernel with five levels (the tiled kernel holds four): 3 x 405 x 1024 = 1,244,160 outputs, on the fp64 pyramid rounded to fp32"""
    from oracle import ops as OO
    B, C, H, W, levels = 3, 32, 32, 32, 5
    f1, f2 = randn(B, C, H, W, seed=1201), randn(B, C, H, W, seed=1202)
    ref = [r.float() for r in allpairs_pyramid(f1, f2, levels)]
    pyr = torch.cat([r.reshape(-1) for r in ref]).to(dev)
    coords = OO.coords_grid(B, H, W) + 3.0 * randn(B, 2, H, W, seed=1203)
    out = filled(dev, B, levels * 81, H, W)
    assert out.numel() > TRIP1
    call("cf_corr_lookup", pyr, coords.to(dev), out, B, H, W, levels, 4)
    print()
    row("flat lookup 3 x 32 x 32, 5 levels (%d > %d)" % (out.numel(), TRIP1), out, OO.corr_lookup(ref, coords, 4), 3e-5, TRIP1)


def test_second_trip_convex_upsample(dev):
    """convex_upsample_kernel (C = 4 takes the flat form): 17 x 64 x 32 x 32 = 1,114,112 items"""
    from oracle import ops as OO
    B, C, h, w = 17, 4, 32, 32
    assert B * 64 * h * w > TRIP1
    flow, mask = randn(B, C, h, w, seed=1211), 2 * randn(B, 576, h, w, seed=1212)
    out = filled(dev, B, C, 8 * h, 8 * w)
    call("cf_convex_upsample", flow.to(dev), mask.to(dev), out, B, C, h, w)
    print()
    row("convex upsample 17 x 4 x 32 x 32 (%d items > %d)" % (B * 64 * h * w, TRIP1), out, OO.convex_upsample(flow, mask), 1e-5)
    row("    samples 16.. (every item of the second trip)", out[16:], OO.convex_upsample(flow[16:], mask[16:]), 1e-5)


def pyramid_rows(dev, tag, B, C, H, W, levels, seed):
    """cf_corr_pyramid into a NaN-filled buffer: every level against fp64 at 3e-5, levels 1.. bit-equal to the pool of the stored level before"""
    from cineflow import ops
    from cineflow._lib import check as lib_check, lib
    f1, f2 = randn(B, C, H, W, seed=seed), randn(B, C, H, W, seed=seed + 1)
    pyr = filled(dev, ops.pyramid_numel(B, H, W, levels))
    f1d, f2d = f1.to(dev), f2.to(dev)
    h = lib()
    h.cf_profile_enable(64)
    try:                                               # the launches booked under PK_ALLPAIRS (7) tell which path the library took
        lib_check(h.cf_profile_reset(), "cf_profile_reset")
        call("cf_corr_pyramid", f1d, f2d, pyr, B, C, H, W, levels)
        ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
        lib_check(h.cf_profile_read(7, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)), "cf_profile_read")
    finally:
        h.cf_profile_enable(0)
    ref = allpairs_pyramid(f1, f2, levels)
    lv, off = [], 0
    for l, r in enumerate(ref):
        lv.append(pyr[off:off + r.numel()].view(r.shape).cpu())
        off += r.numel()
        row("%s level %d (%d x %d)" % (tag, l, H >> l, W >> l), lv[l], r, 3e-5)
        if l:
            assert torch.equal(lv[l], F.avg_pool2d(lv[l - 1], 2, stride=2)), "%s: level %d is not the pool of the stored level %d" % (tag, l, l - 1)
    assert off == pyr.numel()
    return pyr, lv, int(n.value)


def test_second_trip_generic_pyramid(dev):
    """W = 64 keeps the fp32 GEMM + avgpool2x2_kernel path; level 1 is 2 x 2048 x 16 x 32 = 2,097,152 pooled items"""
    B, C, H, W = 2, 32, 32, 64
    assert B * H * W * (H // 2) * (W // 2) > TRIP1
    print()
    launches = pyramid_rows(dev, "generic pyramid 2 x 32 x 32 x 64", B, C, H, W, 4, 1221)[2]
    assert launches >= 4, launches                     # the GEMM and three pooling launches


def test_second_trip_elementwise_gru_binary_copy(dev):
    print()
    B, C, HW = 2, 8, 66001
    n = B * C * HW
    assert n > TRIP1
    gates, h, cand = torch.sigmoid(randn(B, 2 * C, HW, seed=1301)), randn(B, C, HW, seed=1302), torch.tanh(randn(B, C, HW, seed=1303))
    out = filled(dev, B, C, HW)
    call("cf_gru_reset_mul", gates.to(dev), h.to(dev), out, B, C, HW)
    row("gru_reset_mul 2 x 8 x 66001 (%d > %d)" % (n, TRIP1), out, gates[:, :C] * h, 0, TRIP1)
    out = filled(dev, B, C, HW)
    call("cf_gru_blend", gates.to(dev), h.to(dev), cand.to(dev), out, B, C, HW)
    u = gates[:, C:].double()
    want = (1 - u) * h.double() + u * cand.double()
    ratio = ((out.cpu().double() - want).abs() / (2.0 ** -22 * (h.abs() + cand.abs()).double())).reshape(-1)
    ratio_line("gru_blend 2 x 8 x 66001: |diff| / (2^-22 (|h| + |cand|))", float(ratio.max()), 1.0)
    ratio_line("    %d items past %d" % (n - TRIP1, TRIP1), float(ratio[TRIP1:].max()), 1.0)
    assert float(ratio.max()) <= 1.0                                                     # NaN <= 1 is False
    a = randn(3, 352001, seed=1304)
    assert a.numel() > TRIP1
    for op, code, fn in (("add", 0, torch.add), ("sub", 1, torch.sub), ("mul", 2, torch.mul)):
        for period, b in (("b_period < n", randn(352001, seed=1305 + code)), ("b_period == n", randn(3, 352001, seed=1308 + code))):
            out = filled(dev, *a.shape)
            call("cf_binary", code, a.to(dev), b.to(dev), out, a.numel(), b.numel())
            row("binary %s, %s (%d > %d)" % (op, period, a.numel(), TRIP1), out, fn(a, b), 0, TRIP1)
    B, sct, sco, dct, dco, C, HW = 2, 5, 1, 6, 2, 3, 176001
    assert B * C * HW > TRIP1
    src = randn(B, sct, HW, seed=1311)
    for act, code, fn in (("none", 0, lambda t: t), ("relu", 2, F.relu)):
        dst = filled(dev, B, dct, HW)
        call("cf_copy_channels", src.to(dev), sct, sco, dst, dct, dco, B, C, HW, code)
        row("copy_channels %s, 3 of 5 -> 2.. of 6 (%d > %d)" % (act, B * C * HW, TRIP1), dst[:, dco:dco + C], fn(src[:, sco:sco + C]), 0)
        row("    sample 1 (holds the second trip)", dst[1:, dco:dco + C], fn(src[1:, sco:sco + C]), 0)
        assert bool(torch.isnan(dst[:, :dco]).all()) and bool(torch.isnan(dst[:, dco + C:]).all()), "copy_channels wrote outside its slice"


def test_second_trip_elementwise_crop_pad_flip_coords(dev):
    from oracle import ops as OO
    print()
    N, H, W, y0, x0, h, w = 5, 500, 470, 17, 9, 461, 459
    assert N * h * w > TRIP1
    x = randn(N, H, W, seed=1321)
    xd = x.to(dev)
    c = filled(dev, N, h, w)
    call("cf_crop2d", xd, c, N, H, W, y0, x0, h, w)
    row("crop2d 5 x 500 x 470 -> 461 x 459 (%d > %d)" % (N * h * w, TRIP1), c, x[:, y0:y0 + h, x0:x0 + w], 0, TRIP1)
    p = filled(dev, N, H, W)
    call("cf_pad2d", c, p, N, h, w, y0, x0, H, W)
    ref = torch.zeros_like(x)
    ref[:, y0:y0 + h, x0:x0 + w] = x[:, y0:y0 + h, x0:x0 + w]
    row("pad2d back to 500 x 470 (%d > %d)" % (N * H * W, TRIP1), p, ref, 0, TRIP1)
    for fh, fw in ((1, 0), (0, 1), (1, 1)):
        f = filled(dev, N, H, W)
        call("cf_flip2d", xd, f, N, H, W, fh, fw)
        row("flip2d (%d, %d)" % (fh, fw), f, torch.flip(x, [d for d, on in ((1, fh), (2, fw)) if on]), 0, TRIP1)
    B, H, W = 9, 250, 237
    assert B * 2 * H * W > TRIP1
    g = filled(dev, B, 2, H, W)
    call("cf_coords_grid", g, B, H, W)
    row("coords_grid 9 x 250 x 237 (%d > %d)" % (B * 2 * H * W, TRIP1), g, OO.coords_grid(B, H, W), 0, TRIP1)


def test_second_trip_elementwise_tta_tiles_argmax(dev):
    print()
    B, K, H, W = 2, 3, 730, 727
    assert B * H * W > TRIP1
    logits, acc0 = 2 * randn(B, K, H, W, seed=1331), randn(B, K, H, W, seed=1332)
    acc = acc0.clone().to(dev)
    call("cf_tta_accumulate", torch.flip(logits, (2, 3)).contiguous().to(dev), acc, B, K, H, W, 1, 1, 0.7)
    row("tta_accumulate 2 x 3 x 730 x 727, both flips (%d px > %d)" % (B * H * W, TRIP1), acc, acc0.double() + 0.7 * torch.softmax(logits.double(), 1),
        1e-6, TRIP1, channels=True)
    K, X, Y, lx, ly, ph, pw = 3, 640, 600, 17, 9, 600, 590
    assert K * ph * pw > TRIP1
    pred, gauss = randn(K, ph, pw, seed=1333), torch.rand(ph, pw, generator=torch.Generator().manual_seed(1334)) + 0.1
    agg0, cnt0 = randn(K, X, Y, seed=1335), randn(K, X, Y, seed=1336)
    agg, cnt = agg0.clone().to(dev), cnt0.clone().to(dev)
    call("cf_tile_accumulate", pred.to(dev), gauss.to(dev), agg, cnt, K, X, Y, lx, ly, ph, pw)
    ra, rc = agg0.clone(), cnt0.clone()
    ra[:, lx:lx + ph, ly:ly + pw] += pred
    rc[:, lx:lx + ph, ly:ly + pw] += gauss
    row("tile_accumulate 3 x 600 x 590 into 640 x 600 (%d > %d): agg" % (K * ph * pw, TRIP1), agg, ra, 0)
    row("    cnt", cnt, rc, 0)
    row("    class 2 (holds the second trip): agg", agg[2], ra[2], 0)
    X, Y = 1031, 1021
    assert X * Y > TRIP1
    agg, cnt = randn(K, X, Y, seed=1337), torch.rand(K, X, Y, generator=torch.Generator().manual_seed(1338)) + 0.5
    probs, seg = filled(dev, K, X, Y), filled(dev, X, Y, dtype=torch.uint8)
    call("cf_tile_finalize", agg.to(dev), cnt.to(dev), probs, seg, K, X, Y)
    row("tile_finalize 3 x 1031 x 1021 (%d px > %d): probs" % (X * Y, TRIP1), probs, agg / cnt, 0)
    row("    probs of the pixels past %d" % TRIP1, probs.reshape(K, -1)[:, TRIP1:], (agg / cnt).reshape(K, -1)[:, TRIP1:], 0)
    assert torch.equal(seg.cpu().long(), (agg / cnt).argmax(0)), "tile_finalize labels"
    B, K, HW = 2, 5, 530711
    assert B * HW > TRIP1
    x = randn(B, K, HW, seed=1339)
    x[0, 3, :1000], x[0, 1, :1000] = 9.0, 9.0                                            # ties: the first maximum wins
    x[1, 4, -1000:], x[1, 2, -1000:] = 9.0, 9.0
    am = filled(dev, B, HW, dtype=torch.uint8)
    call("cf_argmax_channels", x.to(dev), am, B, K, HW)
    want = x.argmax(1)
    assert int(want[0, 0]) == 1 and int(want[1, -1]) == 2
    bad = am.cpu().long() != want
    ratio_line("argmax_channels 2 x 5 x 530711 (%d > %d): differing" % (B * HW, TRIP1), float(bad.sum()), 0)
    ratio_line("    %d items past %d" % (B * HW - TRIP1, TRIP1), float(bad.reshape(-1)[TRIP1:].sum()), 0)
    assert not bool(bad.any())


def test_second_trip_count_out_of_range(dev):
    """count_out_of_range_kernel: one ballot and one atomic per wave that saw a bad value, under the partly active last wave of the second trip"""
    n, limit = TRIP1 + 3 * 64 + 37, 65504.0
    assert n % 64 == 37
    x = 100.0 * randn(n, seed=1341)
    inside = float(np.nextafter(np.float32(limit), np.float32(0)))
    last_wave = TRIP1 + 3 * 64
    plant = {0: NAN, 63: float("inf"), 64: -limit, 65: inside, 500000: float("-inf"), TRIP1 - 1: limit,           # first trip: 5 bad
             TRIP1: NAN, TRIP1 + 1: -inside, TRIP1 + 70: float("inf"), TRIP1 + 127: limit, TRIP1 + 128: 7e4,       # second trip: 4 bad
             last_wave: float("-inf"), last_wave + 1: inside, last_wave + 35: NAN, n - 1: limit}                   # its last, partial wave: 3 bad
    for i, v in plant.items():
        x[i] = v
    want = int((~(x.abs() < limit)).sum())
    assert want == 12
    xd = x.to(dev)
    print()
    for tag, lo, hi, expect in (("whole", 0, n, 12), ("first trip", 0, TRIP1, 5),
                                ("the tail as its own launch", TRIP1, n, 7), ("the last partial wave alone", last_wave, n, 3)):
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        call("cf_count_out_of_range", xd[lo:hi], hi - lo, limit, counter)
        ratio_line("count_out_of_range %s (n = %d): |count - %d|" % (tag, hi - lo, expect), abs(int(counter.item()) - expect), 0)
        assert int(counter.item()) == expect, (tag, int(counter.item()), expect)


# ================================================================================================= row 3: RAFT maps with H != W
def lookup_coords(B, H, W, seed):
    """grid + an offset field whose x amplitude (0.3 W) and y amplitude (0.08 H) differ, with coordinates planted past each of the four borders"""
    from oracle import ops as OO
    off = randn(B, 2, H, W, seed=seed)
    off[:, 0] *= 0.3 * W
    off[:, 1] *= 0.08 * H
    coords = OO.coords_grid(B, H, W) + off
    coords[:, 0, 0, 0], coords[:, 0, 1, 1], coords[:, 1, 2, 2], coords[:, 1, 3, 3] = -6.5, W + 5.25, -6.75, H + 5.5
    coords[:, :, 4, 4] = torch.tensor([W - 1.0, H - 1.0])                                # exactly the last pixel
    assert float(coords[:, 0].min()) < -4 and float(coords[:, 0].max()) > W + 3 and float(coords[:, 1].min()) < -4 and float(coords[:, 1].max()) > H + 3
    return coords


def tiled_lookup_row(dev, tag, pyr, lv, B, H, W, levels, seed):
    from oracle import ops as OO
    assert (H * W) % 64 == 0 and levels <= 4
    coords = lookup_coords(B, H, W, seed)
    out = filled(dev, B, levels * 81, H, W)
    call("cf_corr_lookup", pyr, coords.to(dev), out, B, H, W, levels, 4)
    row("%s tiled lookup" % tag, out, OO.corr_lookup(lv, coords, 4), 3e-5)
    return coords, out


RAFT_MAPS = [   # route, B, C, H, W, levels
    ("fused", 2, 32, 16, 32, 4),                   # one row group, grid 8
    ("fused", 2, 32, 48, 32, 4),                   # three row groups, H > W, grid 72
    ("fused", 8, 16, 16, 32, 4),                   # one channel chunk, grid 32
    ("W = 32, grid 4: generic", 1, 32, 16, 32, 4),
    ("W = 32, C = 24: generic", 2, 24, 16, 32, 4),
    ("W = 32, 3 levels: generic", 2, 32, 16, 32, 3),
    ("generic", 2, 32, 16, 20, 4),                 # pools 5 -> 2
    ("generic", 2, 32, 8, 24, 3),
]


@pytest.mark.parametrize("route,B,C,H,W,levels", RAFT_MAPS)
def test_raft_maps(dev, route, B, C, H, W, levels):
    # the launcher's own condition (allpairs_pyramid_fused), restated to name the rows; the launch count below is what observes the path
    fused = W == 32 and H % 16 == 0 and C % 16 == 0 and levels == 4 and (B * (H * W // 128) * (H // 16)) % 8 == 0
    assert fused == (route == "fused")
    tag = "%s %d x %d x %d x %d" % (route, B, C, H, W)
    print()
    pyr, lv, launches = pyramid_rows(dev, tag, B, C, H, W, levels, 1400 + 7 * H + W + C + B)
    print("  %s: %d launches booked for the pyramid" % (tag, launches))
    assert (launches == 1) if fused else (launches >= levels), "%s: %d launches: not the path this row is named for" % (tag, launches)
    tiled_lookup_row(dev, tag, pyr, lv, B, H, W, levels, 1450 + H + W)


def test_tiled_lookup_coarsest_2x2(dev):
    B, C, H, W = 2, 32, 16, 16
    print()
    pyr, lv, _ = pyramid_rows(dev, "generic 2 x 32 x 16 x 16", B, C, H, W, 4, 1461)
    assert lv[3].shape[-2:] == (2, 2)
    tiled_lookup_row(dev, "16 x 16, 4 levels, coarsest 2 x 2:", pyr, lv, B, H, W, 4, 1463)


@pytest.mark.parametrize("H,W", [(48, 32), (32, 64)])
def test_tiled_lookup_equals_flat_kernel(dev, H, W):
    """corr.hip says of the tiled lookup: 'same rounding path as the flat kernel'.  A five-level pyramid starts with the four-level one, so
    the flat kernel (five levels) and the tiled one (four) look the same planes up at the same coordinates: channels 0..323 agree bit for bit"""
    from cineflow import ops
    B, C = 1, 32
    f1, f2 = randn(B, C, H, W, seed=1471 + H), randn(B, C, H, W, seed=1472 + H)
    pyr5 = ops.corr_pyramid(f1.to(dev), f2.to(dev), 5)
    n4 = ops.pyramid_numel(B, H, W, 4)
    coords = lookup_coords(B, H, W, 1473 + W).to(dev)
    flat, tiled = filled(dev, B, 5 * 81, H, W), filled(dev, B, 4 * 81, H, W)
    call("cf_corr_lookup", pyr5, coords, flat, B, H, W, 5, 4)
    call("cf_corr_lookup", pyr5[:n4], coords, tiled, B, H, W, 4, 4)
    assert not bool(torch.isnan(flat).any()) and not bool(torch.isnan(tiled).any())
    bad = flat[:, :324] != tiled
    print()
    ratio_line("tiled lookup vs flat kernel %d x %d: differing values" % (H, W), float(bad.sum()), 0)
    assert not bool(bad.any()), "%d of %d values differ, max|diff| %.3e" % (int(bad.sum()), bad.numel(), float((flat[:, :324] - tiled).abs().max()))


# ================================================================================================= row 4: twin-kernel tails, minimum sizes
@pytest.mark.parametrize("H,W,nsteps", [(21, 30, 0), (21, 30, 1), (21, 30, 2), (21, 30, 7), (20, 32, 0), (20, 32, 2)])
def test_vecint_tails(dev, vec_amp, H, W, nsteps):
    """W % 4 != 0: warp_bilinear_2d_kernel with an addend; even nsteps: the ping-pong starts in `out`; nsteps = 0: the scaling alone"""
    from oracle import ops as OO
    vec = vec_amp * randn(3, 2, H, W, seed=1500 + W + nsteps)
    print()
    out = c_vecint(vec.to(dev), nsteps)
    row("vecint 3 x %d x %d, nsteps %d" % (H, W, nsteps), out, OO.vecint(vec.clone(), nsteps), 1e-5)
    if nsteps == 0:
        assert torch.equal(out.cpu(), vec)


@pytest.mark.parametrize("W", [12, 11])
def test_memory_input_widths(dev, W):
    B, H = 3, 10
    x0, xt, cum = randn(B, 1, H, W, seed=1511), randn(B, 1, H, W, seed=1512), 3 * randn(B, 2, H, W, seed=1513)
    print()
    row("memory_input 3 x 10 x %d" % W, c_memory(x0.to(dev), xt.to(dev), cum.to(dev)), memory_ref(x0, xt, cum), 2e-6)


@pytest.mark.parametrize("H,W", [(2, 2), (2, 4), (3, 4), (5, 8), (9, 5)])
def test_small_2d(dev, vec_amp, H, W):
    """the minimum legal sizes (size - 1 = 1 in the coordinate normalisation) and W = 4, where one four-pixel Jacobian thread holds both
    borders of its row: every 2-D entry point"""
    from oracle import ops as OO
    B, C, T, s = 3, 2, 2, 1520 + 10 * H + W
    tag = "%d x %d" % (H, W)
    print()
    flow, src = 0.8 * randn(B, 2, H, W, seed=s), randn(B, C, H, W, seed=s + 1)
    row("warp " + tag, c_warp(flow.to(dev), src.to(dev)), OO.warp_bilinear(flow.clone(), src), 2e-6)
    far = 2.5 * flow
    far[0, 0, 0, 0] = 1e6
    row("warp, far flows " + tag, c_warp(far.to(dev), src.to(dev)), OO.warp_bilinear(far.clone(), src), 2e-5)
    vec = vec_amp * randn(B, 2, H, W, seed=s + 2)
    for nsteps in (2, 7):
        row("vecint %s, nsteps %d" % (tag, nsteps), c_vecint(vec.to(dev), nsteps), OO.vecint(vec.clone(), nsteps), 1e-5)
    fl5, lab = 0.8 * randn(T, B, 2, H, W, seed=s + 3), rand_labels(B, H, W, K=4, seed=s + 4)
    label_row("labels " + tag, c_labels(fl5.to(dev), lab.to(dev), 4), OO.warp_labels(fl5, lab[:, None].float())[:, :, 0])
    label_row("labels, 3 classes " + tag, c_labels(fl5.to(dev), (lab % 3).to(dev), 3), OO.warp_labels(fl5, (lab % 3)[:, None].float(), 3)[:, :, 0])
    x0, xt = randn(B, 1, H, W, seed=s + 5), randn(B, 1, H, W, seed=s + 6)
    row("memory_input " + tag, c_memory(x0.to(dev), xt.to(dev), flow.to(dev)), memory_ref(x0, xt, flow), 2e-6)
    jacobian_row("jacobian " + tag, c_jacobian(far.to(dev)), far)


@pytest.mark.parametrize("D,H,W", [(2, 6, 7), (3, 5, 7), (2, 2, 2)])
def test_small_3d(dev, D, H, W):
    from oracle import ops as OO
    B, C, s = 2, 2, 1600 + 100 * D + 10 * H + W
    tag = "%d x %d x %d" % (D, H, W)
    flow, src = 0.8 * randn(B, 3, D, H, W, seed=s), randn(B, C, D, H, W, seed=s + 1)
    print()
    row("warp 3-D " + tag, c_warp3(flow.to(dev), src.to(dev)), OO.warp_bilinear(flow.clone(), src), 2e-6)
    jacobian_row("jacobian 3-D " + tag, c_jacobian3(flow.to(dev)), flow)


def test_warp_3d_edge_cases(dev):
    """the 3-D twins of test_warp_edge_cases: flows that leave through all six faces, exact integer shifts, one 1e6 entry"""
    from oracle import ops as OO
    D, H, W = 5, 9, 11
    src = randn(3, 2, D, H, W, seed=1701)
    flow = torch.zeros(3, 3, D, H, W)
    flow[0, 0], flow[0, 1], flow[0, 2] = 2.0, -3.0, 5.0                                   # integer shift
    flow[1] = 12.0 * randn(3, D, H, W, seed=1702)                                         # leaves everywhere
    flow[1, :, 0, 0, 0] = 1e6
    flow[2, 0, :2], flow[2, 0, -2:] = -3.5, 3.5                                           # one slab per face
    flow[2, 1, :, :2], flow[2, 1, :, -2:] = -4.25, 4.25
    flow[2, 2, :, :, :3], flow[2, 2, :, :, -3:] = -5.75, 5.75
    out = c_warp3(flow.to(dev), src.to(dev))
    print()
    row("warp 3-D edge cases 5 x 9 x 11", out, OO.warp_bilinear(flow.clone(), src), 2e-5)
    shifted = torch.zeros_like(src[0])
    shifted[:, :D - 2, 3:, :W - 5] = src[0, :, 2:, :H - 3, 5:]
    row("    the integer shift against the moved volume", out[0], shifted, 2e-5)
    for face in (out[2, :, :2, 2:-2, 3:-3], out[2, :, -2:, 2:-2, 3:-3]):                 # z - 3.5 < -1, z + 3.5 > D: nothing to sample
        assert float(face.abs().max()) == 0.0


# ================================================================================================= row 5: misaligned contiguous views
def fenced(t, dev, lead=1):
    """t as a view `lead` elements into a NaN-fenced (255 for uint8) buffer"""
    fill = 255 if t.dtype == torch.uint8 else NAN
    buf = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=dev)
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t.to(dev))
    assert view.data_ptr() % 16 == lead * t.element_size()
    return buf, view


def fences_hold(buf, view, lead=1):
    edge = torch.cat([buf[:lead], buf[lead + view.numel():]])
    return bool((edge == 255).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(edge).all())


def same(a, b):
    """bit for bit (-0.0 is not +0.0)"""
    bits = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def test_misaligned_views(dev, vec_amp):
    """The four-pixel kernels issue 16-byte accesses on flow, source / addend and output (4-byte on the label output); the launchers send
    a tensor that is not on such a boundary to the one-pixel kernels.  Each tensor in turn is a view one element into a fenced buffer: the
    result equals the aligned call's (four-pixel kernel) bit for bit -- the twins' arithmetic is the same -- and the fences stay."""
    from oracle import ops as OO
    B, C, H, W, T = 3, 2, 24, 32, 2
    flow = 3.0 * randn(B, 2, H, W, seed=1801)
    flow[1] *= 12.0                                                                       # leaves every border
    flow[1, :, 0, 0] = 1e6
    flow[2] = torch.round(flow[2])                                                        # exact integer displacements
    src = randn(B, C, H, W, seed=1802)
    fd, sd = flow.to(dev), src.to(dev)
    print()
    base = c_warp(fd, sd)
    row("warp 3 x 2 x 24 x 32, aligned", base, OO.warp_bilinear(flow.clone(), src), 2e-5)
    for which in ("flow", "src", "out"):
        bf, f = fenced(flow, dev) if which == "flow" else (None, fd)
        bs, s = fenced(src, dev) if which == "src" else (None, sd)
        bo, o = fenced(torch.full_like(src, NAN), dev) if which == "out" else (None, None)
        got = c_warp(f, s, o)
        assert same(got, base), "warp, %s misaligned: %d values differ from the aligned call" % (which, int((got != base).sum()))
        for b, v in ((bf, f), (bs, s), (bo, o)):
            assert b is None or fences_hold(b, v), "warp, %s misaligned: fence overwritten" % which
    vec = vec_amp * randn(B, 2, H, W, seed=1803)
    vd = vec.to(dev)
    for nsteps in (2, 3):
        base = c_vecint(vd, nsteps)
        row("vecint nsteps %d, aligned" % nsteps, base, OO.vecint(vec.clone(), nsteps), 1e-5)
        for which in ("vec", "out", "tmp"):
            bv, v = fenced(vec, dev) if which == "vec" else (None, vd)
            bo, o = fenced(torch.full_like(vec, NAN), dev) if which == "out" else (None, None)
            bt, t = fenced(torch.full_like(vec, NAN), dev) if which == "tmp" else (None, None)
            got = c_vecint(v, nsteps, o, t)
            assert same(got, base), "vecint nsteps %d, %s misaligned: %d values differ" % (nsteps, which, int((got != base).sum()))
            for b, w in ((bv, v), (bo, o), (bt, t)):
                assert b is None or fences_hold(b, w), "vecint, %s misaligned: fence overwritten" % which
    base = c_jacobian(fd)
    jacobian_row("jacobian 3 x 24 x 32, aligned", base, flow)
    bd, d = fenced(flow, dev)
    assert same(c_jacobian(d), base) and fences_hold(bd, d), "jacobian, disp misaligned"
    bo, o = fenced(torch.full((B, H, W), NAN, dtype=torch.float64), dev)
    assert o.data_ptr() % 16 == 8
    assert same(c_jacobian(fd, o), base) and fences_hold(bo, o), "jacobian, det misaligned"
    fl5 = torch.stack([flow, 0.5 * flow.flip(0)])
    lab = rand_labels(B, H, W, K=4, seed=1804)
    f5d, ld = fl5.to(dev), lab.to(dev)
    base = c_labels(f5d, ld, 4)
    label_row("labels 2 x 3 x 24 x 32, aligned", base, OO.warp_labels(fl5, lab[:, None].float())[:, :, 0])
    bf, f = fenced(fl5, dev)
    assert same(c_labels(f, ld, 4), base) and fences_hold(bf, f), "labels, flow misaligned"
    bl, l = fenced(lab, dev)
    assert same(c_labels(f5d, l, 4), base) and fences_hold(bl, l), "labels, label input one byte in"
    bo, o = fenced(torch.full((T, B, H, W), 255, dtype=torch.uint8), dev)
    assert o.data_ptr() % 4 == 1
    assert same(c_labels(f5d, ld, 4, o), base) and fences_hold(bo, o), "labels, output one byte in"
