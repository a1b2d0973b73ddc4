"""The fp32 arithmetic of the bilinear-tap kernels, restated on the CPU in numpy float32: csrc/common.h gives csrc/warp.hip, the lookups of
csrc/corr.hip and sample_points_kernel (csrc/elementwise.hip) ONE sequence of individually rounded operations -- st_coord -> make_taps ->
sample_taps -- so every output element has exactly one right bit pattern.  test_tap_chain_cpu.py pins this module (goldens, the oracle,
hand-worked cases, fp64); test_gpu_tap_chains.py holds the kernels to it with `==`.  A plain helper module: no tests live here.

Every array below is float32 and every numpy operation on float32 arrays rounds once to float32, which is what __fadd_rn / __fsub_rn /
__fmul_rn / __fdiv_rn do under `fp contract(off)`.  Nothing here calls torch arithmetic or grid_sample.

  st_coord     loc = i + f;  g = 2 (loc / (S - 1) - 0.5);  pos = ((g + 1) / 2) (S - 1)
  make_taps    yf = floor y;  wy = y - yf;  ey = 1 - wy  (same for x);  the floor clamped to [-2, size + 1] BEFORE the integer conversion
               (NaN -> -2, as fmaxf gives);  w00 = ex ey, w01 = wx ey, w10 = ex wy, w11 = wx wy;  a tap is valid when its row and column
               lie inside the image and `fin`: y and x not NaN and |.| < 1e9
  sample_taps  ((a w00 + b w01) + c w10) + d w11 with an invalid tap's value 0 and THE MULTIPLY PERFORMED: 0 x NaN = NaN, so a
               non-finite coordinate (NaN weights) gives NaN, a far finite one (finite weights) gives 0
  labels       per class k the sum ((s00 + s01) + s10) + s11 with sNN = wNN where the tap is valid and carries label k, else +0; the first
               strictly greater sum wins from best = -1, so non-finite and far flows give class 0
  3-D          its own weights ((f + 1) - c) and (c - f) taken before the clamp, products (wx wy) wz, corners tnw .. bse accumulated from
               +0 with invalid corners SKIPPED: non-finite flows give 0

Variants (resolving power: each is the chain with exactly one change; `variant=` on every function):
  contracted      the tap sum as fma(d, w11, fma(c, w10, fma(b, w01, a w00))) (3-D: acc = fma(v, w, acc)), fma32 from _fma_chain.py
  pairwise        (a w00 + b w01) + (c w10 + d w11)
  corner_weights  the 2-D weights formed as the 3-D kernel forms its own: ey = (yf + 1) - y instead of 1 - (y - yf)
  last_tie        the label argmax taking >=

The second half of the module is the table of inputs that test_gpu_tap_chains.py runs on the device and on which test_tap_chain_cpu.py
shows that every variant differs from the chain.
"""
import numpy as np
import torch

from _fma_chain import fma32

F32 = np.float32
ONE, TWO, HALF = F32(1), F32(2), F32(0.5)
VARIANTS_2D = ("contracted", "pairwise", "corner_weights")
NAN, INF = float("nan"), float("inf")


def _np(t, dtype=F32):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert dtype is None or a.dtype == dtype, a.dtype
    return a


# ===================================================================================================== common.h
def st_coord(idx, f, size_m1):
    idx, f, s = np.asarray(idx, dtype=F32), np.asarray(f), F32(size_m1)
    assert f.dtype == F32
    with np.errstate(all="ignore"):
        loc = idx + f
        g = TWO * (loc / s - HALF)
        return ((g + ONE) / TWO) * s


def make_taps(y, x, H, W, variant=None):
    """y, x float32 arrays of one shape -> dict of y0, x0 (int32), w00 .. w11 (float32) and v00 .. v11 (bool), all of that shape"""
    assert y.dtype == F32 and x.dtype == F32 and y.shape == x.shape
    with np.errstate(all="ignore"):
        yf, xf = np.floor(y), np.floor(x)
        wy, wx = y - yf, x - xf
        if variant == "corner_weights":
            ey, ex = (yf + ONE) - y, (xf + ONE) - x
        else:
            ey, ex = ONE - wy, ONE - wx
        # fminf(fmaxf(v, -2), size + 1): np.fmax / np.fmin return the other operand for a NaN, like fmaxf / fminf
        y0 = np.fmin(np.fmax(yf, F32(-2)), F32(H) + ONE).astype(np.int32)
        x0 = np.fmin(np.fmax(xf, F32(-2)), F32(W) + ONE).astype(np.int32)
        t = {"y": y, "x": x, "y0": y0, "x0": x0, "w00": ex * ey, "w01": wx * ey, "w10": ex * wy, "w11": wx * wy}
        fin = (y == y) & (x == x) & (np.abs(y) < F32(1e9)) & (np.abs(x) < F32(1e9))
    y0v, y1v = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    x0v, x1v = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    t["v00"], t["v01"], t["v10"], t["v11"] = fin & y0v & x0v, fin & y0v & x1v, fin & y1v & x0v, fin & y1v & x1v
    assert all(v.dtype == F32 for k, v in t.items() if k[0] == "w")
    return t


TAP_NAMES = (("a", "v00", 0, 0), ("b", "v01", 0, 1), ("c", "v10", 1, 0), ("d", "v11", 1, 1))


def gather_taps(planes, t, W, invalid=0):
    """planes [G, C, H * W], taps of shape [G, P] -> the four tap values [G, C, P]; an invalid tap issues no load and is `invalid`"""
    G, C, HW = planes.shape
    base = t["y0"].astype(np.int64) * W + t["x0"]
    out = {}
    for name, v, dy, dx in TAP_NAMES:
        ok = t[v]
        off = np.where(ok, base + dy * W + dx, 0)
        assert off.min() >= 0 and off.max() < HW
        val = np.take_along_axis(planes, np.broadcast_to(off[:, None, :], (G, C, off.shape[1])), axis=2)
        out[name] = np.where(ok[:, None, :], val, planes.dtype.type(invalid))
    return out


def tap_sum(g, t, variant=None):
    a, b, c, d = g["a"], g["b"], g["c"], g["d"]
    w00, w01, w10, w11 = (t[k][:, None, :] for k in ("w00", "w01", "w10", "w11"))
    with np.errstate(all="ignore"):
        if variant == "contracted":
            return fma32(d, w11, fma32(c, w10, fma32(b, w01, a * w00)))
        if variant == "pairwise":
            return (a * w00 + b * w01) + (c * w10 + d * w11)
        return ((a * w00 + b * w01) + c * w10) + d * w11


def sample_taps(planes, y, x, H, W, variant=None):
    """planes [G, C, H * W] sampled at y, x [G, P] -> (values [G, C, P], detail: the chain's intermediates, each [G, P] or [G, C, P])"""
    t = make_taps(y, x, H, W, variant)
    g = gather_taps(planes, t, W)
    out = tap_sum(g, t, variant)
    assert out.dtype == F32
    detail = dict(t)
    detail.update(g)
    detail["result"] = out
    return out, detail


def explain(detail, index):
    """the chain's intermediates at one output element (index into [G, C, P]), as one line"""
    g, c, p = (int(v) for v in index)
    parts = ["%s=%r" % (k, detail[k][g, p].item()) for k in ("y", "x", "y0", "x0", "w00", "w01", "w10", "w11")]
    parts += ["%s=%r%s" % (k, detail[k][g, c, p].item(), "" if detail[v][g, p] else "(invalid)") for k, v, _, _ in TAP_NAMES]
    return ", ".join(parts + ["result=%r" % detail["result"][g, c, p].item()])


# ===================================================================================================== warp.hip, 2-D
def _pixel_coords(flow, H, W):
    """flow [G, 2, H, W] -> sampling positions y, x [G, H * W]"""
    ii, jj = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    y = st_coord(ii[None], flow[:, 0], H - 1)
    x = st_coord(jj[None], flow[:, 1], W - 1)
    return y.reshape(len(flow), H * W), x.reshape(len(flow), H * W)


def warp2d(flow, src, addend=None, variant=None, detail=False):
    """cf_warp_bilinear_2d: flow [B, 2, H, W], src [B, C, H, W] -> [B, C, H, W]; with `addend` [B, C, H, W] the result is addend + v"""
    flow, src = _np(flow), _np(src)
    B, C, H, W = src.shape
    assert flow.shape == (B, 2, H, W)
    y, x = _pixel_coords(flow, H, W)
    out, det = sample_taps(src.reshape(B, C, H * W), y, x, H, W, variant)
    if addend is not None:
        with np.errstate(all="ignore"):
            out = _np(addend).reshape(B, C, H * W) + out
        det["result"] = out
    out = out.reshape(B, C, H, W)
    return (out, det) if detail else out


def vecint2d(vec, nsteps, variant=None, detail=False):
    """cf_vecint_2d: scale by 1.0f / (1 << nsteps), then nsteps times cur = cur + warp(cur, cur); detail is the last step's"""
    cur = _np(vec) * (ONE / F32(1 << nsteps))
    det = None
    for _ in range(nsteps):
        cur, det = warp2d(cur, cur, addend=cur, variant=variant, detail=True)
    assert cur.dtype == F32
    return (cur, det) if detail else cur


def warp_labels2d(flow, labels, K, variant=None, detail=False):
    """cf_warp_labels_2d: flow [T, B, 2, H, W] float32, labels [B, H, W] uint8 -> uint8 [T, B, H, W]"""
    flow, labels = _np(flow), _np(labels, np.uint8)
    T, B, _, H, W = flow.shape
    assert flow.shape[2] == 2 and labels.shape == (B, H, W)
    y, x = _pixel_coords(flow.reshape(T * B, 2, H, W), H, W)
    t = make_taps(y, x, H, W, variant if variant == "corner_weights" else None)
    lab = labels.reshape(B, 1, H * W).astype(np.int32)[np.arange(T * B) % B]              # tb % B
    g = gather_taps(lab, t, W, invalid=-1)
    best, arg = np.full((T * B, H * W), F32(-1)), np.zeros((T * B, H * W), dtype=np.uint8)
    zero = F32(0)
    for k in range(K):
        s = [np.where(g[n][:, 0] == k, t[w], zero) for n, w in (("a", "w00"), ("b", "w01"), ("c", "w10"), ("d", "w11"))]
        with np.errstate(all="ignore"):
            v = ((s[0] + s[1]) + s[2]) + s[3]
        win = (v >= best) if variant == "last_tie" else (v > best)
        best, arg = np.where(win, v, best), np.where(win, np.uint8(k), arg)
    out = arg.reshape(T, B, H, W)
    if detail:
        t.update({n: g[n] for n in "abcd"})
        t["result"] = arg[:, None, :]
        return out, t
    return out


def memory_input(x0, xt, cum, variant=None, detail=False):
    """cf_memory_input: x0, xt [B, 1, H, W], cum [B, 2, H, W] -> [B, 6, H, W]: x0, xt, cum, x0 - reg, reg with reg = warp(cum, xt)"""
    x0, xt, cum = _np(x0), _np(xt), _np(cum)
    reg, det = warp2d(cum, xt, variant=variant, detail=True)
    with np.errstate(all="ignore"):
        out = np.concatenate([x0, xt, cum, x0 - reg, reg], axis=1)
    assert out.dtype == F32
    return (out, det) if detail else out


def sample_points(field, pts, variant=None, detail=False):
    """cf_sample_points_2d: field [B, C, H, W], pts [B, 2, P] (x, y in pixels) -> [B, C, P]"""
    field, pts = _np(field), _np(pts)
    B, C, H, W = field.shape
    assert pts.shape[:2] == (B, 2)
    with np.errstate(all="ignore"):
        gx = TWO * (pts[:, 0] / F32(W - 1) - HALF)
        gy = TWO * (pts[:, 1] / F32(H - 1) - HALF)
        xs = ((gx + ONE) / TWO) * F32(W - 1)
        ys = ((gy + ONE) / TWO) * F32(H - 1)
    out, det = sample_taps(field.reshape(B, C, H * W), ys, xs, H, W, variant)
    return (out, det) if detail else out


def corr_lookup(pyramid, coords, radius, variant=None, detail=False):
    """cf_corr_lookup: pyramid = list of [B, N, H >> l, W >> l] (N = H W), coords [B, 2, H, W] (x, y) -> [B, L D D, H, W] with D = 2 r + 1
    and channel l D D + i D + j sampled at (x 2^-l + (i - r), y 2^-l + (j - r)); detail: one dict per level, of shape [B N, 1, D D]"""
    coords = _np(coords)
    B, _, H, W = coords.shape
    N, D, r = H * W, 2 * radius + 1, radius
    off = np.arange(-r, r + 1).astype(F32)
    out, dets = [], []
    for l, lev in enumerate(pyramid):
        lev = _np(lev)
        Hl, Wl = H >> l, W >> l
        assert lev.shape == (B, N, Hl, Wl)
        inv = ONE / F32(1 << l)
        with np.errstate(all="ignore"):
            cx = (coords[:, 0].reshape(B * N, 1) * inv) + off[None]                       # [B N, D] over i
            cy = (coords[:, 1].reshape(B * N, 1) * inv) + off[None]                       # [B N, D] over j
            gx = (TWO * cx) / F32(Wl - 1) - ONE
            gy = (TWO * cy) / F32(Hl - 1) - ONE
            x = ((gx + ONE) / TWO) * F32(Wl - 1)
            y = ((gy + ONE) / TWO) * F32(Hl - 1)
        xx = np.ascontiguousarray(np.broadcast_to(x[:, :, None], (B * N, D, D))).reshape(B * N, D * D)
        yy = np.ascontiguousarray(np.broadcast_to(y[:, None, :], (B * N, D, D))).reshape(B * N, D * D)
        v, det = sample_taps(lev.reshape(B * N, 1, Hl * Wl), yy, xx, Hl, Wl, variant)
        out.append(v.reshape(B, N, D * D).transpose(0, 2, 1).reshape(B, D * D, H, W))
        dets.append(det)
    out = np.ascontiguousarray(np.concatenate(out, axis=1))
    return (out, dets) if detail else out


# ===================================================================================================== warp.hip, 3-D
def warp3d(flow, src, variant=None, detail=False):
    """cf_warp_trilinear_3d: flow [B, 3, D, H, W], src [B, C, D, H, W] -> [B, C, D, H, W]; detail: positions and floors per axis [B, V],
    the eight weights and validities [B, V] and the eight corner values [B, C, V] (V = D H W)"""
    assert variant in (None, "contracted")
    flow, src = _np(flow), _np(src)
    B, C, D, H, W = src.shape
    assert flow.shape == (B, 3, D, H, W)
    V = D * H * W
    zz, yy, xx = np.meshgrid(np.arange(D, dtype=F32), np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    pos, lo, hi, i0, ok = [], [], [], [], []
    with np.errstate(all="ignore"):
        for ax, (grid, size) in enumerate(((zz, D), (yy, H), (xx, W))):
            c = st_coord(grid[None], flow[:, ax], size - 1).reshape(B, V)
            f = np.floor(c)
            hi.append(c - f)                                                              # weight of the corner at f + 1
            lo.append((f + ONE) - c)                                                      # weight of the corner at f
            k = np.fmin(np.fmax(f, F32(-2)), F32(size) + ONE).astype(np.int64)
            i0.append(k)
            ok.append(((k >= 0) & (k < size), (k + 1 >= 0) & (k + 1 < size)))
            pos.append(c)
        planes = src.reshape(B, C, V)
        acc = np.zeros((B, C, V), dtype=F32)
        det = {"pos": pos, "i0": i0, "w": [], "v": [], "val": []}
        for k in range(8):                                                                # tnw, tne, tsw, tse, bnw, bne, bsw, bse
            dz, dy, dx = k >> 2, (k >> 1) & 1, k & 1
            w = ((hi[2] if dx else lo[2]) * (hi[1] if dy else lo[1])) * (hi[0] if dz else lo[0])
            v = ok[0][dz] & ok[1][dy] & ok[2][dx]
            off = np.where(v, (i0[0] + dz) * (H * W) + (i0[1] + dy) * W + (i0[2] + dx), 0)
            val = np.take_along_axis(planes, np.broadcast_to(off[:, None, :], (B, C, V)), axis=2)
            nxt = fma32(val, w[:, None, :], acc) if variant == "contracted" else acc + val * w[:, None, :]
            acc = np.where(v[:, None, :], nxt, acc)
            det["w"].append(w), det["v"].append(v), det["val"].append(val)
    assert acc.dtype == F32
    det["result"] = acc
    out = acc.reshape(B, C, D, H, W)
    return (out, det) if detail else out


def explain3d(detail, index):
    """the 3-D chain's intermediates at one output element (index into [B, C, V]), as one line"""
    b, c, p = (int(v) for v in index)
    parts = ["%s=%r (floor %d)" % (n, detail["pos"][a][b, p].item(), detail["i0"][a][b, p]) for a, n in enumerate("zyx")]
    for k, n in enumerate(("tnw", "tne", "tsw", "tse", "bnw", "bne", "bsw", "bse")):
        ok = bool(detail["v"][k][b, p])
        parts.append("%s: w=%r v=%s" % (n, detail["w"][k][b, p].item(), repr(detail["val"][k][b, c, p].item()) if ok else "(skipped)"))
    return ", ".join(parts + ["result=%r" % detail["result"][b, c, p].item()])


def vecint3d(vec, nsteps):
    """cineflow.ops.vecint on a 3-D field: the scaling, then v = v + warp3d(v, v) per step"""
    cur = _np(vec) * (ONE / F32(1 << nsteps))
    with np.errstate(all="ignore"):
        for _ in range(nsteps):
            cur = cur + warp3d(cur, cur)
    return cur


# ===================================================================================================== the shared input table
def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def rand_labels(*shape, K, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * K).to(torch.uint8).numpy()


LEAVE = (0.5, 3.25, 7.75, 11.0)                         # how far the `sides` flows leave the image, per border row / column
FAR = (1e6, 9.9e8, 1.1e9, 3e38)                         # finite, gives 0: in the image's terms far away; the last two fail the `fin` guard
NONFINITE = (NAN, INF, -INF)


def warp_flows(B, H, W, seed):
    """name -> flow [B, 2, H, W].  Sample 0 carries the pattern; samples 1.. stay 3 x unit normal, so every entry also has pixels with
    four in-image taps and fractional weights (where an FMA or another association shows).  H >= 12, W >= 16."""
    base = 3.0 * randn(B, 2, H, W, seed=seed)
    ii, jj = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    t = {"normal3": base.copy()}
    f = base.copy()
    f[0] = 0.0
    for k, d in enumerate(LEAVE):                        # position -d, H - 1 + d, W - 1 + d: every side left by 0.5 to 11 pixels
        f[0, 0, k], f[0, 0, H - 1 - k] = -k - d, k + d
        f[0, 1, :, k], f[0, 1, :, W - 1 - k] = -k - d, k + d
    t["sides"] = f
    f = base.copy()
    f[0] = np.round(f[0])
    t["integers"] = f
    f = base.copy()
    f[0] = np.round(f[0]) + 0.5
    f[0, 1, H // 2:] = np.round(f[0, 1, H // 2:])        # lower half: half-integer rows, integer columns
    t["halves"] = f
    f = base.copy()
    f[0, 0], f[0, 1] = H - 1 - ii, W - 1 - jj            # exactly row H - 1 and column W - 1
    f[0, 1, H // 2:] = 0.25                              # lower half: the last row alone
    t["last"] = f
    f = base.copy()
    for k, v in enumerate(FAR):
        f[0, 0, 1, 2 + k], f[0, 1, 3, 2 + k], f[0, 0, 5, 2 + k], f[0, 1, 7, 2 + k] = v, v, -v, -v
        f[0, :, 9, 2 + 2 * k] = v
    t["far"] = f
    f = base.copy()
    for k, v in enumerate(NONFINITE):                    # one pixel each, in each flow channel; three neighbours of one row, three apart
        f[0, 0, 2, 4 + k], f[0, 1, 5 + 3 * k, 9 + k] = v, v
    t["nonfinite"] = f
    assert all(v.dtype == F32 and v.shape == (B, 2, H, W) for v in t.values())
    return t


def nonfinite_pixels(H, W):
    """(channel, i, j) of the planted pixels of warp_flows(...)['nonfinite'], sample 0"""
    return [(0, 2, 4 + k) for k in range(3)] + [(1, 5 + 3 * k, 9 + k) for k in range(3)]


# cf_warp_bilinear_2d rows: name -> (B, C, H, W, view); view: the source, flow and output one float into a larger buffer
WARP_ROWS = {
    "v4 2x3x17x24": (2, 3, 17, 24, False),
    "one-pixel 2x3x17x23": (2, 3, 17, 23, False),
    "one-pixel 2x3x17x24, views one float in": (2, 3, 17, 24, True),
    "v4 2x1x17x24": (2, 1, 17, 24, False),
    "v4 2x5x17x24": (2, 5, 17, 24, False),
    "one-pixel 2x5x17x23": (2, 5, 17, 23, False),
}


def warp_row_inputs(name):
    B, C, H, W, _ = WARP_ROWS[name]
    return warp_flows(B, H, W, seed=2000 + 10 * W + C), randn(B, C, H, W, seed=2001 + 10 * W + C)


# cf_vecint_2d rows: name -> (B, H, W, nsteps, NaN pixel or None); amplitude 3.0, that of the golden fixtures
VECINT_ROWS = {}
for _H, _W in ((20, 32), (21, 30)):
    for _n in (0, 1, 2, 7):
        VECINT_ROWS["3x%dx%d nsteps %d" % (_H, _W, _n)] = (3, _H, _W, _n, None)
    VECINT_ROWS["3x%dx%d nsteps 2, one NaN" % (_H, _W)] = (3, _H, _W, 2, (1, 0, 9, 14))
VECINT_ROWS["1x256x256 nsteps 7"] = (1, 256, 256, 7, None)


def vecint_row_inputs(name):
    B, H, W, nsteps, nan_at = VECINT_ROWS[name]
    vec = (3.0 * randn(B, 2, H, W, seed=2100 + H + W)).astype(F32)
    if nan_at is not None:
        vec[nan_at] = NAN
    return vec, nsteps


# cf_warp_labels_2d rows: name -> (T, B, K, H, W, output byte offset)
LABEL_ROWS = {
    "v4<4> K=4 16x32": (3, 2, 4, 16, 32, 0),
    "v4<0> K=2 16x32": (3, 2, 2, 16, 32, 0),
    "v4<0> K=3 16x32": (3, 2, 3, 16, 32, 0),
    "v4<0> K=8 16x32": (3, 2, 8, 16, 32, 0),
    "one-pixel K=4 16x30": (3, 2, 4, 16, 30, 0),
    "one-pixel K=3 16x30": (3, 2, 3, 16, 30, 0),
    "one-pixel K=4 16x32, output one byte in": (3, 2, 4, 16, 32, 1),
}


def label_row_inputs(name):
    """-> flow [T, B, 2, H, W] and two label maps [B, H, W]: random, and a two-class checkerboard.  Frame 0: 3 x unit normal with the
    non-finite and far pixels; frame 1: half-integer flows (every pixel of the checkerboard is then a tie of two classes at 0.5 or, in
    the lower half where the columns move by integers, of two taps at 0.5); frame 2: 3 x unit normal."""
    T, B, K, H, W, _ = LABEL_ROWS[name]
    assert T == 3
    flows = warp_flows(B, H, W, seed=2200 + W + K)
    flow = np.stack([flows["nonfinite"], flows["halves"], flows["normal3"]])
    flow[1, 1] = flows["halves"][0]                                                       # both samples of frame 1 carry the pattern
    for k, v in enumerate(FAR):
        flow[0, 1, 0, 11, 3 + k], flow[0, 1, 1, 12, 3 + k] = v, -v
    random = rand_labels(B, H, W, K=K, seed=2201 + W + K)
    assert int(random.max()) == K - 1
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lo, hi = (1 if K > 2 else 0), K - 1
    checker = np.where((ii + jj) % 2 == 0, lo, hi).astype(np.uint8)
    checker = np.stack([checker, np.where((ii + jj) % 2 == 0, hi, lo).astype(np.uint8)][:B])
    return np.ascontiguousarray(flow), random, checker


# cf_memory_input rows: name -> (B, H, W)
MEMORY_ROWS = {"3x20x32": (3, 20, 32), "3x21x30": (3, 21, 30)}


def memory_row_inputs(name):
    B, H, W = MEMORY_ROWS[name]
    return randn(B, 1, H, W, seed=2300 + W), randn(B, 1, H, W, seed=2301 + W), warp_flows(B, H, W, seed=2302 + W)


def sample_points_inputs():
    """field [2, 3, 9, 13], pts [2, 2, 257] (x, y): uniform over the image and a margin, then points exactly on pixels, on the last row and
    column, outside on every side, far away and non-finite"""
    B, C, H, W, P = 2, 3, 9, 13, 257
    field = randn(B, C, H, W, seed=2400)
    u = torch.rand(B, 2, P, generator=torch.Generator().manual_seed(2401)).numpy()
    pts = np.empty((B, 2, P), dtype=F32)
    pts[:, 0], pts[:, 1] = u[:, 0] * (W + 3) - 2, u[:, 1] * (H + 3) - 2
    plant = [(0.0, 0.0), (5.0, 3.0), (12.0, 8.0), (12.0, 2.5), (4.5, 8.0), (W - 1.0, H - 1.0), (-0.5, 4.0), (3.0, -0.75), (12.5, 4.0), (3.0, 8.25),
             (-3.0, -3.0), (20.0, 20.0), (1e6, 2.0), (2.0, -9.9e8), (1.1e9, 2.0), (2.0, 3e38), (NAN, 2.0), (2.0, NAN), (INF, 2.0), (2.0, -INF),
             (-INF, INF), (NAN, NAN)]
    for k, (px, py) in enumerate(plant):
        pts[k % B, 0, 7 + 3 * k], pts[k % B, 1, 7 + 3 * k] = px, py
    return field, pts


# cf_corr_lookup rows: name -> (B, C, H, W, levels, radius, tiled)
LOOKUP_ROWS = {
    "flat radius 3, 2x16x16x16, 4 levels": (2, 16, 16, 16, 4, 3, False),
    "flat radius 4, 2x16x6x10 (H W % 64 = 60), 2 levels": (2, 16, 6, 10, 2, 4, False),
    "tiled<16> radius 4, 2x16x8x8, 2 levels": (2, 16, 8, 8, 2, 4, True),
    "tiled<16> radius 4, 2x16x16x16, 4 levels": (2, 16, 16, 16, 4, 4, True),
}


def lookup_row_inputs(name):
    """-> features f1, f2 [B, C, H, W] and coords [B, 2, H, W] (x, y): the grid + 3 x unit normal, with pixels sent off every side"""
    B, C, H, W, levels, radius, tiled = LOOKUP_ROWS[name]
    assert tiled == (radius == 4 and levels <= 4 and (H * W) % 64 == 0)                   # cf_corr_lookup's own condition
    assert (H >> (levels - 1)) >= 2 and (W >> (levels - 1)) >= 2
    f1, f2 = randn(B, C, H, W, seed=2500 + H + W), randn(B, C, H, W, seed=2501 + H + W)
    ii, jj = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    coords = np.stack([jj, ii])[None] + 3.0 * randn(B, 2, H, W, seed=2502 + H + W)
    coords[:, 0, 0, 0], coords[:, 0, 1, 1], coords[:, 1, 2, 2], coords[:, 1, 3, 3] = -6.5, W + 5.25, -6.75, H + 5.5
    coords[:, :, 4, 4] = np.array([W - 1.0, H - 1.0], dtype=F32)
    coords[:, :, 5, 5] = np.array([3.0, 2.0], dtype=F32)
    return f1, f2, np.ascontiguousarray(coords.astype(F32))


def warp3d_inputs():
    """name -> flow [2, 3, 5, 9, 7]; and the source [2, 2, 5, 9, 7]"""
    B, C, D, H, W = 2, 2, 5, 9, 7
    src = randn(B, C, D, H, W, seed=2600)
    base = 2.0 * randn(B, 3, D, H, W, seed=2601)
    t = {"normal2": base.copy()}
    f = base.copy()
    f[0] = 0.0
    f[0, 0, :2], f[0, 0, -2:] = -3.5, 3.5                                                 # one slab per face
    f[0, 1, :, :2], f[0, 1, :, -2:] = -4.25, 4.25
    f[0, 2, :, :, :2], f[0, 2, :, :, -2:] = -5.75, 5.75
    t["sides"] = f
    f = base.copy()
    for ax in range(3):
        for k, v in enumerate(NONFINITE + FAR):
            f[0, ax, 1 + ax, 1 + k, 2] = v
    t["nonfinite"] = f
    return t, src


def nonfinite_voxels():
    """(z, y, x) of the planted voxels of warp3d_inputs()[0]['nonfinite'], sample 0: every one samples nothing -> 0"""
    return [(1 + ax, 1 + k, 2) for ax in range(3) for k in range(len(NONFINITE + FAR))]
