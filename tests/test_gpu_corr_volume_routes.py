"""cf_corr_volume on every kernel it can launch, each row held to an fp64 reference of its own arithmetic and to the route probe.

entry point -> kernel -> rows
  cf_corr_volume, cf_corr_volume_route == 2   corr_volume_mfma_kernel<1|2|4> (csrc/corr_mfma.hip)   MFMA_ROWS, test_mfma_aligned_views,
                                                                                                    test_amplitudes, test_non_finite
  cf_corr_volume, cf_corr_volume_route == 1   corr_volume_p7_kernel<1|2|4> (csrc/corr.hip)          P7_ROWS (the first six at the MFMA shapes under
                                                                                                    cf_corr_mfma_enable(0)), test_amplitudes, test_non_finite
  cf_corr_volume, cf_corr_volume_route == 0   corr_volume_generic_kernel (csrc/corr.hip)            GENERIC_ROWS, test_non_finite
cf_corr_volume dispatches on cf_corr_volume_route itself; every row asks the probe first and fails if it names another kernel than the row
does, so a probe that declines (a changed shape rule, a lost alignment) cannot turn an MFMA row into "p7 equals p7".

Every row.  The C ABI writes into a NaN-filled output that lies 64 floats inside a buffer of sentinels; the sentinels on both sides must
be untouched, an element no kernel wrote is NaN, and all samples are compared.  Elements whose displacement leaves the map (A == 0) must
be exactly 0.  The 1e-5 of test_gpu_ops.py against the true result stays beside the bar of the route:

  MFMA         |out - y4| <= SPLIT_BAR x A = 2^-18 A, y4 = (1/C) sum (ch + cl)(ph + pl) over the f16 hi/lo halves the kernel stages, A the
               same sum over the halves' magnitudes (_kernel_refs.corr_volume_refs).  Derivation as in the convolution tables
               (test_gpu_conv_f16s_routes.py): the products are exact, each of the C / 8 <= 32 accumulating instructions rounds once, the
               product with fl(1/C) adds 2 u A.
  p7, generic  |out - true| <= (C + 3) x 2^-24 x A1, A1 = (1/C) sum |c||p|: the certain bound of a C-term fp32 FMA chain plus the rounding
               of 1/C and of the final product (p7) or division (generic).

Each row also shows that its bar resolves: the reference less its last channel fails it on every row, and on MFMA rows hi x hi alone
(y1) and y4 less the lo x hi terms of its last eight channels fail it too.  On the CPU (test_kernel_refs_cpu.py, unit normals, multiples of
2^-18 A): hi x hi only 32 - 124, lo x hi of 8 channels 6.4 - 68, one channel 1.5e4 - 1.4e5, lo x lo 0.005 - 0.023 (not resolvable, not
asserted), y4 - true 0.007 - 0.035.  The old 1e-5 sits at about 1.5 x the worst lo x hi term of one chunk at C = 256: it sees such a drop
only in the tail of a row.

What the rows reach (B, C, H, W, S):
  MFMA  (1,16,8,64,1) (1,16,16,64,2) (1,16,32,64,4)     the minimum of each dilation: one tile row, every halo row outside the map, all S x S
                                                        residue classes, 1 / 2 / 4 tiles, seven or more empty XCD bands (the early return)
        (2,32,16,128,1) (3,48,32,128,2)                 neighbours on all four sides, two / three samples, 4 and 6 chunks, ragged tile count (24)
        (2,256,8,64,1)                                  32 chunks, the longest accumulation
        (300,16,8,64,1) (150,16,16,64,2) (75,16,32,64,4)  300 tiles > the CU count: workgroups with one and with two tiles, the chunk stream
                                                        crosses tile and sample boundaries
        (1,16,16,64,1) (1,16,8,128,1)                   tiles_y = 2, tiles_x = 1 and the reverse: every row above has tiles_y == tiles_x, where
                                                        decode() cannot confuse the two (mutation 6)
        (2,32,16,128,1) as 16-byte-aligned views        four NaN floats before and after each input
  p7    the first six MFMA rows                         both tiled kernels held to independent references at one shape
        (1,8,7,64,1)                                    one step in the whole launch
        (2,5,9,12,2) (2,12,20,40,4)                     channel tails, W < 64, ragged class rows
        (150,24,8,64,1) (150,8,8,64,1) (75,24,16,64,2) (38,8,32,64,4)   300 / 300 / 300 / 304 tiles (tiles_y = 2): 3 and 6 steps in one
                                                        launch, 1 and 2 in another: the odd tail of the staging loop with tile_end
  generic (2,16,8,64,1) r 4, pointers % 16 == 4         the MFMA / p7 shape one float into a NaN-fenced buffer
        (2,5,7,9,2) r 4                                 W % 4 != 0
        (1,4,6,10) r 0 s 1, r 8 s 1, r 4 s 3            1 plane, 289 planes, a dilation outside {1, 2, 4}
        (2,4,81,82,1) r 4                               1,076,004 outputs: a second grid-stride trip

Measured on the MI355X (pytest -s prints one line per row), worst |out - reference| over the row's bar:
  MFMA     minima 0.041 / 0.040 / 0.046; (2,32,16,128,1) 0.051, as fenced views 0.051; (3,48,32,128,2) 0.058; (2,256,8,64,1) 0.038;
           300-tile rows 0.057 / 0.066 / 0.056; (1,16,16,64,1) 0.043; (1,16,8,128,1) 0.043.  max|out - true| <= 2.7e-7 everywhere.
  p7       at the six MFMA shapes 0.153 / 0.168 / 0.176 / 0.133 / 0.111 / 0.016; (1,8,7,64,1) 0.327; (2,5,9,12,2) 0.331; (2,12,20,40,4) 0.288;
           300-tile rows 0.198 / 0.350 / 0.202 / 0.358: no hang, no unwritten element with odd step counts.  max|out - true| <= 3.0e-7.
  generic  misaligned 0.187; (2,5,7,9,2) 0.334; radius 0 / 8 / stride 3: 0.198 / 0.280 / 0.241; (2,4,81,82,1) 0.408, 0.378 over the 27,428
           outputs past 1,048,576.
  amplitudes, (2,64,16,64,1): both bars hold at all three (MFMA 0.041 / 0.041 / 0.043, p7 0.067 / 0.066 / 0.064 of the bar).
           max|out - true| / A (no bar; 2^-24 = 6.0e-8):     cur x 300, prev x 1e-3     x 1e-2, x 1e-2     x 30, x 30
               MFMA                                               1.7e-5                 2.7e-6            1.7e-7
               p7                                                 2.7e-7                 2.6e-7            2.6e-7
           The MFMA route leaves fp32 class below O(1): lo = fp16(x - hi) is an f16 subnormal for |x| < 0.125 and keeps its absolute
           2^-24 resolution only.  The split-exact reference has the same halves, so the bar still holds; csrc/corr_mfma.hip says so now.
  non-finite, (2,16,16,64,2): all three routes produce the oracle's NaN set (72 outputs of the prev element -- dy = -4 leaves the map --
           and the 81 of the cur pixel), the rest at 0.047 (MFMA) / 0.209 (p7, generic) of the bar.  With 7e4 in prev p7 and generic
           stay finite at 0.212; the MFMA route's non-finite outputs lie inside the read-set.

Findings.
  1. corr_volume_generic_kernel wrote 0 for a displacement that leaves the map without reading cur; the oracle and both tiled kernels
     compute cur x 0, so a NaN in cur gave 81 NaNs on an aligned pointer and 45 fewer on a misaligned one (test_non_finite[0]: "45 outputs
     are NaN in the oracle only" on the kernel as it was).  The generic kernel now accumulates cur x 0.
  2. corr_mfma.hip said "C % 8 == 0"; the probe requires C % 16.  Header corrected.
  3. The MFMA route is not fp32 class on operands far below O(1) (table above).  Documented, no bar.

Mutations (scratch builds, every access kept inside its buffer; "old" = the standing corr tests of test_gpu_ops.py):
  1. a_part from kg >> 1 (A = [ah ah al al]: 2 ah bh + 2 al bl)      every MFMA row, view row, amplitudes, non_finite[2] at 1.0e5 - 2.6e5 x
                                                                      the bar; old: 11 fail at 0.3 - 1.6 absolute.  Not subtle: the old tests see it.
  2. hi_off not swapped on odd rows                                   nothing fails, old or new, and nothing can: with a_part / b_part unchanged
                                                                      the K = 32 sum holds the same four products in another order.  The swap is
                                                                      a bank-conflict measure (equivalent mutant).
  3. epilogue px >= r -> px > r                                        every MFMA row (NaN / stale LDS at the missing dx), amplitudes,
                                                                      non_finite[2]; old: 12 fail
  4. MFMA setup() without the -4 S halo offset in x                   every MFMA row, amplitudes, non_finite[2]; old: 12 fail
  5. p7 invC from C rounded up to 8                                   test_p7_rows[2-5-9-12-2] (7.9e5 x), [2-12-20-40-4] (2.8e5 x); old: the
                                                                      four rows of test_corr_volume_radius4 with C % 8 != 0
  6. decode(): ty = id % tiles_x                                      test_mfma_rows[1-16-16-64-1] alone among the MFMA rows (unwritten tile row:
                                                                      NaN), every p7 row with two tile rows (10 of 13), amplitudes,
                                                                      non_finite[1]; old: 17 fail.  (Only the modulus was changed: with
                                                                      the division changed too the sample index leaves the batch.)
  7. (added) cur lo halves of the first chunk of every tile set to 0: the subtle kind, one chunk's lo x hi and lo x lo terms
                                                                      every MFMA row at 6.9 (C = 256) - 95 x the bar, amplitudes 25 x,
                                                                      non_finite[2]; old: 12 fail, 3.0e-4 at C = 16 but 1.9e-5 at
                                                                      (2, 256, 64, 64, 1) and (70, 256, 64, 64, 1): 1.9 x the old 1e-5
  -. the generic kernel as it was                                     test_non_finite[0]

Bench (the generic kernel's device code changed; default bench, frames/s, parent | this tree, alternating):
  771.46 | 770.16, 769.45 | 769.71, 769.56 | 769.60
"""
import contextlib

import pytest
import torch

from _kernel_refs import corr_volume_refs, ratio_line
from _split_exact import SPLIT_BAR

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12345.5                         # the fence around the output
PAD = 64                                # floats of fence on each side: keeps the output 16-byte aligned
TRIP1 = 4096 * 256                      # outputs of the first grid-stride trip of corr_volume_generic_kernel
ROUTE = {0: "generic", 1: "p7", 2: "MFMA"}


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@contextlib.contextmanager
def mfma(on):
    from cineflow._lib import lib
    before = lib().cf_corr_mfma_enable(on)
    try:
        yield
    finally:
        lib().cf_corr_mfma_enable(before)


def device_input(x, dev, lead):
    """lead None: a tensor of its own; else a contiguous view `lead` floats into a buffer with NaNs before and after (4: still 16-byte
    aligned, 1: pointer % 16 == 4).  A read outside x poisons the output."""
    if lead is None:
        xd = x.to(dev)
        assert xd.data_ptr() % 16 == 0
        return xd
    buf = torch.full((x.numel() + lead + (4 if lead == 4 else 7),), NAN, device=dev)
    xd = buf[lead:lead + x.numel()].view(x.shape)
    xd.copy_(x.to(dev))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == (4 * lead) % 16 and bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + x.numel():]).all())
    return xd


def run(dev, route, cur, prev, radius, S, lead=None):
    """probe, then the C ABI into a fenced NaN-filled output -> float64 result on the CPU"""
    from cineflow import ops
    from cineflow._lib import check, lib
    B, C, H, W = cur.shape
    cd, pd = device_input(cur, dev, lead), device_input(prev, dev, lead)
    probe = ops.corr_volume_route(cd, pd, radius, S)
    assert probe == route, "%s, radius %d, dilation %d: the probe names the %s kernel, the row is for the %s kernel" % (
        tuple(cur.shape), radius, S, ROUTE.get(probe, probe), ROUTE[route])
    n = B * (2 * radius + 1) ** 2 * H * W
    buf = torch.full((n + 2 * PAD,), SENT, device=dev)
    out = buf[PAD:PAD + n]
    out.fill_(NAN)
    assert out.data_ptr() % 16 == 0
    check(lib().cf_corr_volume(cd.data_ptr(), pd.data_ptr(), out.data_ptr(), B, C, H, W, radius, S, torch.cuda.current_stream().cuda_stream), "cf_corr_volume")
    host = buf.cpu()
    assert bool((host[:PAD] == SENT).all()) and bool((host[PAD + n:] == SENT).all()), "%s kernel wrote outside its output" % ROUTE[route]
    assert all(torch.equal(d.cpu().view(torch.int32), h.view(torch.int32)) for d, h in ((cd, cur), (pd, prev))), "an input changed"
    return host[PAD:PAD + n].view(B, (2 * radius + 1) ** 2, H, W).double()


_REFS = {}


def refs_of(cur, prev, radius, S, key=None):
    """corr_volume_refs; rows that share inputs (both tiled kernels at one shape) share the reference, which nobody modifies"""
    if key is None:
        return corr_volume_refs(cur, prev, radius, S)
    if key not in _REFS:
        _REFS[key] = corr_volume_refs(cur, prev, radius, S)
    return _REFS[key]


def inputs(B, C, H, W, S, radius=4):
    seed = 7000 + 131 * B + 17 * C + 5 * H + 3 * W + S + 11 * radius
    return randn(B, C, H, W, seed=seed), randn(B, C, H, W, seed=seed + 1)


def judge(tag, route, got, r, C, where=None, resolves=True, first=None, abs_bar=1e-5):
    """the row's bar over `where` (default: everywhere), exact zeros where A == 0, the standing 1e-5 (an absolute figure for O(1) features:
    abs_bar=None on scaled operands), and that the bar resolves (resolves="channel": one channel only, not the lo terms)"""
    A, A1 = r["A"], r["A1"]
    where = torch.ones_like(A, dtype=torch.bool) if where is None else where
    zero = (A == 0) & where
    live = (A > 0) & where
    assert not bool((where & ~(zero | live)).any())
    assert int(live.sum()) > 0
    nz = got[zero]
    assert bool((nz == 0).all()), "%s: %d of %d outputs whose displacement leaves the map are not 0 (NaN: never written)" % (
        tag, int((~(nz == 0)).sum()), nz.numel())
    if route == 2:
        want, bar = r["y4"], SPLIT_BAR * A
    else:
        want, bar = r["true"], (C + 3) * 2.0 ** -24 * A1
    ratio = torch.where(live, (got - want).abs() / bar, torch.zeros_like(bar))
    worst = float(ratio.max()) if not bool(torch.isnan(ratio).any()) else NAN
    ratio_line("%s %s: |out - %s| / bar" % (ROUTE[route], tag, "y4" if route == 2 else "true"), worst, 1.0)
    if first is not None:
        flat = ratio.reshape(-1)
        assert flat.numel() > first
        ratio_line("    %d outputs past %d" % (flat.numel() - first, first), float(flat[first:].max()), 1.0)
    absd = float((got - r["true"])[where].abs().max())
    if abs_bar is not None:
        ratio_line("    max|out - true|", absd, abs_bar)
    assert worst <= 1.0, "%s %s: %.3f x its bar at %s (NaN: an element no kernel wrote)" % (ROUTE[route], tag, worst, "the worst element")
    assert abs_bar is None or absd <= abs_bar, "%s %s: max|out - true| %.3e > %.0e" % (ROUTE[route], tag, absd, abs_bar)
    if resolves:
        over = lambda d: float(torch.where(live, d.abs() / bar, torch.zeros_like(bar)).max())
        assert over(r["d_last"]) > 1, "%s: the bar does not resolve one channel" % tag
        if route == 2 and resolves is True:
            assert over(r["y1"] - r["y4"]) > 1 and over(r["d_lohi8"]) > 1, "%s: the bar does not resolve the lo terms (%.2f, %.2f)" % (
                tag, over(r["y1"] - r["y4"]), over(r["d_lohi8"]))
    return worst


def table_row(dev, route, B, C, H, W, S, radius=4, lead=None, share=False, first=None):
    cur, prev = inputs(B, C, H, W, S, radius)
    tag = "%d x %d x %d x %d, dilation %d%s" % (B, C, H, W, S, "" if radius == 4 else ", radius %d" % radius)
    got = run(dev, route, cur, prev, radius, S, lead)
    r = refs_of(cur, prev, radius, S, key=(B, C, H, W, S, radius) if share else None)
    print()
    return judge(tag, route, got, r, C, first=first)


# ========================================================================================================================= MFMA
SHARED = [(1, 16, 8, 64, 1), (1, 16, 16, 64, 2), (1, 16, 32, 64, 4), (2, 32, 16, 128, 1), (3, 48, 32, 128, 2), (2, 256, 8, 64, 1)]
MANY_TILES_MFMA = [(300, 16, 8, 64, 1), (150, 16, 16, 64, 2), (75, 16, 32, 64, 4)]
MFMA_ROWS = SHARED + MANY_TILES_MFMA + [(1, 16, 16, 64, 1), (1, 16, 8, 128, 1)]


@pytest.mark.parametrize("B,C,H,W,S", MFMA_ROWS)
def test_mfma_rows(dev, B, C, H, W, S):
    if (B, C, H, W, S) in MANY_TILES_MFMA:
        ntiles, cus = B * S * (H // S // 8) * (W // 64), torch.cuda.get_device_properties(dev).multi_processor_count
        assert ntiles > cus, "%d tiles on %d CUs: no workgroup walks two tiles, the row tests nothing it is here for" % (ntiles, cus)
    with mfma(1):
        table_row(dev, 2, B, C, H, W, S, share=(B, C, H, W, S) in SHARED)


def test_mfma_aligned_views(dev):
    """both inputs as 16-byte-aligned views with four NaN floats before and four after: the halo loads of the first and last tile stay inside"""
    with mfma(1):
        table_row(dev, 2, 2, 32, 16, 128, 1, lead=4, share=True)


# ========================================================================================================================= p7
MANY_TILES_P7 = [(150, 24, 8, 64, 1), (150, 8, 8, 64, 1), (75, 24, 16, 64, 2), (38, 8, 32, 64, 4)]
P7_ROWS = SHARED + [(1, 8, 7, 64, 1), (2, 5, 9, 12, 2), (2, 12, 20, 40, 4)] + MANY_TILES_P7


@pytest.mark.parametrize("B,C,H,W,S", P7_ROWS)
def test_p7_rows(dev, B, C, H, W, S):
    if (B, C, H, W, S) in MANY_TILES_P7:
        ntiles = B * S * (((H + S - 1) // S + 6) // 7) * ((W + 63) // 64)
        # 256 is the workgroup count of the p7 launch in cf_corr_volume (csrc/corr.hip: `nwg = nt >= 256 ? 256 : ...`, a constant, not the
        # device's CU count as on the MFMA route): with more tiles than that some workgroups walk two tiles of 1 or 3 chunks.  If that
        # line ever takes the CU count from the device, this assertion has to follow it.
        assert ntiles in (300, 304) and ntiles > 256 and -(-C // 8) in (1, 3)
    with mfma(0):
        table_row(dev, 1, B, C, H, W, S, share=(B, C, H, W, S) in SHARED)


# ========================================================================================================================= generic
GENERIC_ROWS = [(2, 16, 8, 64, 4, 1, 1, None), (2, 5, 7, 9, 4, 2, None, None), (1, 4, 6, 10, 0, 1, None, None), (1, 4, 6, 10, 8, 1, None, None),
                (1, 4, 6, 10, 4, 3, None, None), (2, 4, 81, 82, 4, 1, None, TRIP1)]


@pytest.mark.parametrize("B,C,H,W,radius,S,lead,first", GENERIC_ROWS)
def test_generic_rows(dev, B, C, H, W, radius, S, lead, first):
    if first is not None:
        assert B * (2 * radius + 1) ** 2 * H * W > first
    table_row(dev, 0, B, C, H, W, S, radius=radius, lead=lead, first=first)


# ========================================================================================================================= amplitudes
@pytest.mark.parametrize("sc,sp", [(300.0, 1e-3), (1e-2, 1e-2), (30.0, 30.0)])
def test_amplitudes(dev, sc, sp):
    """(2, 64, 16, 64, 1) with cur, prev scaled: both bars are relative to A, so they hold at every amplitude; below O(1) the lo halves
    are f16 subnormals, the same ones in the reference's split.  The rows go through judge() like the table rows, less two things on
    purpose: the 1e-5 against the true result is an absolute figure for O(1) features and does not apply to scaled operands, and
    the lo-term resolution (y1, d_lohi8) is asserted at x 30 only -- at x 1e-2 and at prev x 1e-3 the subnormal lo halves carry less than
    the bar (that is the finding: y4 itself is 2.7e-6 A and 1.7e-5 A from the true result there), one channel is still resolved.
    max|out - true| / A of both routes is printed (no bar: module docstring)."""
    B, C, H, W, S = 2, 64, 16, 64, 1
    cur, prev = inputs(B, C, H, W, S)
    cur, prev = cur * sc, prev * sp
    r = corr_volume_refs(cur, prev, 4, S)
    live = r["A"] > 0
    print()
    for route in (2, 1):
        with mfma(route == 2):
            got = run(dev, route, cur, prev, 4, S)
        judge("cur x %g, prev x %g" % (sc, sp), route, got, r, C, resolves=True if min(sc, sp) >= 1 else "channel", abs_bar=None)
        print("      max|out - true| / A = %.3e (2^-24 = 6.0e-8)" % float(((got - r["true"]).abs() / r["A"])[live].max()))


# ========================================================================================================================= non-finite
@pytest.mark.parametrize("route", [2, 1, 0])
def test_non_finite(dev, route):
    """(2, 16, 16, 64, 2): one NaN at an interior prev element of sample 0, one NaN at a cur element of sample 1 within 4 S of the border.
    The NaN outputs are the fp32 oracle's, element for element, on every route (the generic kernel through the misaligned view: the
    result of a call must not depend on the alignment of its pointers), every other element meets the row's bar.  Then 7e4, above the
    f16 range, in place of the prev NaN: the fp32 kernels stay finite and inside their bar; the MFMA kernel's hi half is Inf, and all
    that is asserted of it is that every non-finite output lies in the oracle's read-set of that element (include/cineflow.h)."""
    from oracle import ops as OO
    B, C, H, W, S = 2, 16, 16, 64, 2
    cur, prev = inputs(B, C, H, W, S)
    cur[1, 3, 2, 61] = NAN                                     # y = 2 < 4 S and x = 61 >= W - 4 S: displacements leave through two borders
    lead = 1 if route == 0 else None
    print()
    p_nan = prev.clone()
    p_nan[0, 5, 8, 30] = NAN
    reads = torch.isnan(OO.corr_volume(cur, p_nan, 4, S))       # the outputs that read either planted element
    assert int(reads[0].sum()) == 72 and int(reads[1].sum()) == 81 and bool(reads[1, :, 2, 61].all())      # rows 8 - 2 dy: dy = -4 leaves the map
    with mfma(route == 2):
        got = run(dev, route, cur, p_nan, 4, S, lead)
    bad = torch.isnan(got) != reads
    assert not bool(bad.any()), "%s: %d outputs are NaN where the oracle is not, or the reverse (of them %d NaN in the oracle only)" % (
        ROUTE[route], int(bad.sum()), int((bad & reads).sum()))
    judge("NaN in prev and cur", route, got, corr_volume_refs(cur, p_nan, 4, S), C, where=~reads, resolves=False)

    p_big = prev.clone()
    p_big[0, 5, 8, 30] = 7e4
    want_nan = torch.isnan(OO.corr_volume(cur, p_big, 4, S))    # the cur NaN alone
    assert int(want_nan.sum()) == 81
    with mfma(route == 2):
        got = run(dev, route, cur, p_big, 4, S, lead)
    r = corr_volume_refs(cur, p_big, 4, S)
    if route == 2:
        stray = ~torch.isfinite(got) & ~reads
        assert not bool(stray.any()), "MFMA: %d non-finite outputs outside the read-set of the 7e4 element" % int(stray.sum())
        assert bool(torch.isnan(got[want_nan]).all())
        judge("7e4 in prev, outside its read-set", route, got, r, C, where=~reads, resolves=False)
    else:
        assert torch.equal(torch.isnan(got), want_nan) and bool(torch.isfinite(got[~want_nan]).all())
        # the standing 1e-5 does not apply to outputs that hold a 7e4 term: judge them by the bar alone
        live = ~want_nan & (r["A"] > 0)
        worst = float(((got - r["true"]).abs() / ((C + 3) * 2.0 ** -24 * r["A1"]))[live].max())
        ratio_line("%s 7e4 in prev: |out - true| / bar" % ROUTE[route], worst, 1.0)
        assert worst <= 1.0 and bool((got[~want_nan & (r["A"] == 0)] == 0).all())
