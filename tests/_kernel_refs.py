"""Plain numpy / scipy / torch-fp64 restatements of the operators around the convolutions (preprocessing, metrics, the 3-D sliding
window, the Swin window attention, the RAFT all-pairs pyramid and CorrVolume), each a few lines.  The GPU tables test_gpu_preprocess_kernels.py,
test_gpu_metrics_kernels.py, test_gpu_volume_ops.py, test_gpu_window_attention.py, test_gpu_flow_op_shapes.py and
test_gpu_corr_volume_routes.py hold the HIP kernels to these; test_kernel_refs_cpu.py pins every restatement
to the oracle (and through it to the reference's golden vectors) so that helper and kernel cannot be wrong together.
The label-resize references (linear_chain_f64, label_resize_exact) are pinned by test_label_resize_refs_cpu.py and describe the
decision that test_gpu_label_resize.py holds the device to through the oracle."""
import numpy as np
import torch
import torch.nn.functional as F


def ratio_line(tag, worst, bar):
    """one printed line per row (pytest -s): the worst measured figure over its bar"""
    r = worst / bar if bar else (0.0 if worst == 0 else float("inf"))
    print("  %-58s worst %.3e  bar %.1e  ratio %.3f" % (tag, worst, bar, r))
    return r


# ------------------------------------------------------------------------------------------------ cropping
def nonzero_fill_holes(data):
    """cropping.py:25-32: OR over the channels of data != 0 (NaN != 0 holds, -0.0 != 0 does not), then scipy's binary_fill_holes on
    the array as given: (C, X, Y, Z) fills 3-D cavities only, (C, X, Y) fills 2-D holes."""
    from scipy.ndimage import binary_fill_holes
    data = np.asarray(data)
    return binary_fill_holes(np.any(data != 0, axis=0))


def bbox(mask):
    """cropping.py:47-55 -> [[min, max + 1]] per axis; an empty mask raises ValueError like np.min of an empty sequence"""
    co = np.nonzero(np.asarray(mask))
    return [[int(c.min()), int(c.max()) + 1] for c in co]


def seg_outside_mask(seg, mask, label):
    """cropping.py:128-135: seg[(seg == 0) & (mask == 0)] = label, the mask broadcast over seg's channels"""
    seg = np.array(seg, copy=True)
    seg[(seg == 0) & (np.asarray(mask)[None] == 0)] = label
    return seg


# ------------------------------------------------------------------------------------------------ normalisation
def masked_moments(x, seg=None, lo=None, hi=None):
    """(count, sum x, sum x^2, sum |x|) over the voxels with seg >= 0 and lo < x < hi (strict), fp64 sums of the fp32 values"""
    x = np.asarray(x, np.float32).ravel()
    sel = np.ones(x.shape, bool)
    if seg is not None:
        sel &= np.asarray(seg).ravel() >= 0
    if lo is not None:
        sel &= (x > np.float32(lo)) & (x < np.float32(hi))
    v = x[sel].astype(np.float64)
    return int(v.size), float(v.sum()), float((v * v).sum()), float(np.abs(v).sum())


def normalize_f32(x, sub, div, clip=None, seg=None, zero_outside=False):
    """((clip ? np.clip(x, lo, hi) : x) - float32(sub)) / float32(div) in float32; voxels with seg < 0 become 0 when zero_outside"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        y = np.clip(x, np.float32(clip[0]), np.float32(clip[1])) if clip is not None else x
        y = ((y - np.float32(sub)) / np.float32(div)).astype(np.float32)
    if zero_outside:
        y = np.where(np.asarray(seg) < 0, np.float32(0), y)
    return y


# ------------------------------------------------------------------------------------------------ metrics
def confusion(test, reference, K):
    """K x K int64 matrix M[t, r] = #voxels with test label t and reference label r"""
    t, r = np.asarray(test).ravel().astype(np.int64), np.asarray(reference).ravel().astype(np.int64)
    return np.bincount(t * K + r, minlength=K * K).reshape(K, K)


def surface_border(mask):
    """medpy's border: mask ^ binary_erosion(mask, face structure) -> sorted (z, y, x) rows (z = 0 for a 2-D mask)"""
    from scipy.ndimage import binary_erosion, generate_binary_structure
    m = np.asarray(mask).astype(bool)
    co = np.argwhere(m ^ binary_erosion(m, structure=generate_binary_structure(m.ndim, 1), iterations=1))
    co = np.concatenate([np.zeros((len(co), 3 - m.ndim), co.dtype), co], 1)
    return co[np.lexsort(co.T[::-1])]


def region_stats(x, lab, K):
    """per label k < K: (sum x, count, #(x < 0), sum |x|) in fp64; labels >= K are ignored"""
    x, lab = np.asarray(x, np.float64).ravel(), np.asarray(lab).ravel()
    return np.array([[x[lab == k].sum(), (lab == k).sum(), (x[lab == k] < 0).sum(), np.abs(x[lab == k]).sum()] for k in range(K)])


# ------------------------------------------------------------------------------------------------ resampling
def cubic_axis(x, axis, m):
    """skimage.transform.resize(order=3, mode='edge') along one axis = scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True), fp64"""
    from scipy.ndimage import zoom
    x = np.asarray(x, np.float64)
    z = [1.0] * x.ndim
    z[axis] = m / float(x.shape[axis])
    out = zoom(x, z, order=3, mode="nearest", grid_mode=True)
    assert out.shape[axis] == m
    return out


def slab_minmax(x):
    """x [C, A, S, B] -> (min, max) of every slab (c, s), each [C, S]"""
    x = np.asarray(x)
    return x.min(axis=(1, 3)), x.max(axis=(1, 3))


def slab_clip_f32(y, mn=None, mx=None):
    """y [C, A, S, B] fp64 clipped to its slab's range (when given) and rounded to float32"""
    y = np.asarray(y, np.float64)
    if mn is not None:
        y = np.clip(y, mn[:, None, :, None], mx[:, None, :, None])
    return y.astype(np.float32)


def resize_edge(x, new_shape, linear):
    """x [N, X, Y, Z] -> [N, *new_shape], fp64: per axis src = (n / n2) (dst + 0.5) - 0.5; linear between the two edge-clamped
    neighbours, or nearest = floor(src + 0.5) edge-clamped."""
    x = np.asarray(x, np.float64)
    for ax, (n2, lin) in enumerate(zip(new_shape, linear), 1):
        n = x.shape[ax]
        s = (float(n) / n2) * (np.arange(n2) + 0.5) - 0.5
        if lin:
            f = np.floor(s)
            w = (s - f).reshape([-1 if a == ax else 1 for a in range(x.ndim)])
            i0, i1 = np.clip(f.astype(int), 0, n - 1), np.clip(f.astype(int) + 1, 0, n - 1)
            x = np.take(x, i0, ax) * (1.0 - w) + np.take(x, i1, ax) * w
        else:
            x = np.take(x, np.clip(np.floor(s + 0.5).astype(int), 0, n - 1), ax)
    return x


def _chain_axes(shape, new_shape, linear):
    """per axis the support of one output sample: (indices [taps, n2], fp64 weights [taps, n2]); a linear axis has the two edge-clamped
    neighbours of s = (n / n2) (o + 0.5) - 0.5 with weights (1 - y, y), y = s - floor(s); a nearest axis has one tap of weight 1"""
    axes = []
    for n, n2, lin in zip(shape, new_shape, linear):
        s = (float(n) / n2) * (np.arange(n2) + 0.5) - 0.5              # numpy rounds every product and sum on its own
        if lin:
            f = np.floor(s)
            y = s - f
            i = f.astype(np.int64)
            axes.append((np.stack([np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1)]), np.stack([1.0 - y, y])))
        else:
            axes.append((np.clip(np.floor(s + 0.5).astype(np.int64), 0, n - 1)[None], np.ones((1, n2))))
    return axes


def linear_chain_f64(x, new_shape, linear):
    """scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True) of a 2-D or 3-D array restated as one fp64 chain, bit for bit
    (test_label_resize_refs_cpu.py): t += ((v * w_a) * w_b) * w_c over the 2^d support points, last axis fastest, every product and
    sum rounded on its own.  An axis with linear = 0 is nearest (floor(s + 0.5), edge-clamped) as in resize_edge."""
    import itertools
    x = np.asarray(x, np.float64)
    assert x.ndim == len(new_shape) == len(linear) and x.ndim in (2, 3)
    axes = _chain_axes(x.shape, new_shape, linear)
    t = np.zeros(tuple(int(v) for v in new_shape))
    for taps in itertools.product(*[range(len(a[0])) for a in axes]):
        c = x[np.ix_(*[a[0][k] for a, k in zip(axes, taps)])]
        for d, (a, k) in enumerate(zip(axes, taps)):
            c = c * a[1][k].reshape([-1 if e == d else 1 for e in range(x.ndim)])
        t = t + c
    return t


def labels_from_chain(seg, new_shape, linear):
    """batchgenerators' resize_segmentation(order=1) on linear_chain_f64: labels ascending, each assigned where its indicator >= 0.5"""
    seg = np.asarray(seg)
    out = np.zeros(tuple(int(v) for v in new_shape), seg.dtype)
    for c in np.unique(seg):
        out[linear_chain_f64(seg == c, new_shape, linear) >= 0.5] = c
    return out


def label_resize_exact(seg, new_shape, linear):
    """The same decision in exact integer arithmetic.  s = (n (2o + 1) - n2) / (2 n2), so a linear axis' weights are (2 n2 - r, r) / (2 n2)
    with r = (n (2o + 1) - n2) mod 2 n2, and indicator * D is an integer for D = prod 2 n2.
    -> (labels present, sign of indicator - 1/2 per label [L, *new_shape] int8, tie mask (some label's indicator is exactly 1/2),
    smallest non-zero |indicator - 1/2|).  A nearest axis must not sit on a rounding boundary (asserted)."""
    import itertools
    seg = np.asarray(seg)
    assert seg.ndim == len(new_shape) == len(linear)
    D, axes = 1, []
    for n, n2, lin in zip(seg.shape, new_shape, linear):
        n, n2 = int(n), int(n2)
        num = n * (2 * np.arange(n2, dtype=np.int64) + 1) - n2           # s = num / (2 n2)
        if lin:
            f, r = num // (2 * n2), num % (2 * n2)
            axes.append((np.stack([np.clip(f, 0, n - 1), np.clip(f + 1, 0, n - 1)]), np.stack([2 * n2 - r, r])))
            D *= 2 * n2
        else:
            i = np.clip((num + n2) // (2 * n2), 0, n - 1)
            s = (float(n) / n2) * (np.arange(n2) + 0.5) - 0.5
            assert np.array_equal(i, np.clip(np.floor(s + 0.5).astype(np.int64), 0, n - 1)), "a nearest axis rounds differently in fp64"
            axes.append((i[None], np.ones((1, n2), np.int64)))
    assert 2 * D < 2 ** 62, "indicator * D does not fit int64"
    labels = np.unique(seg)
    sign = np.zeros((len(labels),) + tuple(int(v) for v in new_shape), np.int8)
    gap = None
    for j, c in enumerate(labels):
        t = np.zeros(sign.shape[1:], np.int64)
        ind = (seg == c).astype(np.int64)
        for taps in itertools.product(*[range(len(a[0])) for a in axes]):
            v = ind[np.ix_(*[a[0][k] for a, k in zip(axes, taps)])]
            for d, (a, k) in enumerate(zip(axes, taps)):
                v = v * a[1][k].reshape([-1 if e == d else 1 for e in range(seg.ndim)])
            t += v
        diff = 2 * t - D                                                 # (indicator - 1/2) * 2 D
        sign[j] = np.sign(diff)
        nz = np.abs(diff[diff != 0])
        if nz.size:
            gap = int(nz.min()) if gap is None else min(gap, int(nz.min()))
    return labels, sign, (sign == 0).any(0), (gap / (2.0 * D) if gap is not None else float("inf"))


def resize3d_f32_chain(x, new_shape, linear):
    """cf_resize3d's arithmetic (postprocess.hip resize3d_kernel) in numpy fp32, without FMA contraction: coordinates in double,
    weight rounded to fp32, nested lerp u + (v - u) * w along z, then y, then x.  x [X, Y, Z] -> fp32 [*new_shape]."""
    x = np.asarray(x, np.float32)
    idx, w = [], []
    for n, n2, lin in zip(x.shape, new_shape, linear):
        s = (float(n) / n2) * (np.arange(n2) + 0.5) - 0.5
        if lin:
            f = np.floor(s)
            i = f.astype(np.int64)
            idx.append((np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1)))
            w.append((s - f).astype(np.float32))
        else:
            i = np.clip(np.floor(s + 0.5).astype(np.int64), 0, n - 1)
            idx.append((i, i))
            w.append(np.zeros(n2, np.float32))
    for ax in (2, 1, 0):
        wa = w[ax].reshape([-1 if e == ax else 1 for e in range(3)])
        u, v = np.take(x, idx[ax][0], ax), np.take(x, idx[ax][1], ax)
        x = (u + ((v - u) * wa).astype(np.float32)).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------ sliding window
def flip(x, flags):
    """torch.flip over the trailing axes whose flag is set"""
    nd = x.dim()
    dims = [nd - len(flags) + a for a, f in enumerate(flags) if f]
    return torch.flip(x, dims) if dims else x.clone()


def tta_softmax(logits):
    """what mirroring TTA converges to when every mirrored pass sees the mirrored logits: the fp64 softmax over the channels"""
    return torch.softmax(logits.double(), 1)


def tile_add(agg, cnt, pred, gauss, corner):
    """agg[:, tile] += pred, cnt[:, tile] += gauss (1 when absent), in the tensors' own precision"""
    sl = (slice(None),) + tuple(slice(c, c + p) for c, p in zip(corner, pred.shape[1:]))
    agg[sl] += pred
    cnt[sl] += gauss if gauss is not None else 1.0
    return agg, cnt


# ------------------------------------------------------------------------------------------------ Swin window attention
def window_attention(q, k, v, bias_table, heads, ws, shift, mask=True):
    """q, k, v [B, C, H, W], bias_table [(2 ws - 1)^2, heads] -> [B, C, H, W], all in fp64: roll by -shift, partition into ws x ws
    windows, softmax(scale q k^T + bias_table[relative index] + (-100 between border regions of the rolled map)) v, reverse, roll back."""
    q, k, v, bias_table = (t.double() for t in (q, k, v, bias_table))
    B, C, H, W = v.shape
    hd, N = C // heads, ws * ws

    def part(t):
        t = torch.roll(t, (-shift, -shift), (2, 3)) if shift else t
        t = t.reshape(B, heads, hd, H // ws, ws, W // ws, ws).permute(0, 3, 5, 1, 4, 6, 2)     # B, wy, wx, head, ty, tx, d
        return t.reshape(B, H // ws, W // ws, heads, N, hd)

    ty, tx = np.divmod(np.arange(N), ws)
    rel = (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + (tx[:, None] - tx[None, :] + ws - 1)
    bias = bias_table[torch.from_numpy(rel).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    attn = (hd ** -0.5) * part(q) @ part(k).transpose(-1, -2) + bias
    if shift and mask:
        def region(n):
            r = np.zeros(n, np.int64)
            r[n - ws:n - shift], r[n - shift:] = 1, 2
            return r
        reg = torch.from_numpy(3 * region(H)[:, None] + region(W)[None, :])
        reg = reg.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(H // ws, W // ws, N)
        attn = attn + torch.where(reg[..., :, None] != reg[..., None, :], -100.0, 0.0).double()[None, :, :, None]
    o = torch.softmax(attn, -1) @ part(v)                                                     # B, wy, wx, head, N, hd
    o = o.reshape(B, H // ws, W // ws, heads, ws, ws, hd).permute(0, 3, 6, 1, 4, 2, 5).reshape(B, C, H, W)
    return torch.roll(o, (shift, shift), (2, 3)) if shift else o


# ------------------------------------------------------------------------------------------------ point sampling
def sample_points(field, pts):
    """SpatialTransformerContour (integration.py:5-34): field [B, C, H, W], pts [B, 2, P] (channel 0 along W, 1 along H) -> [B, C, P]
    through F.grid_sample(align_corners=True, padding_mode='zeros') in the dtype of `field`."""
    B, C, H, W = field.shape
    p = pts.to(field.dtype)
    gx = 2 * (p[:, 0] / (W - 1) - 0.5)
    gy = 2 * (p[:, 1] / (H - 1) - 0.5)
    grid = torch.stack([gx, gy], -1)[:, :, None, :]                                           # B, P, 1, 2
    return F.grid_sample(field, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0]


# ------------------------------------------------------------------------------------------------ RAFT all-pairs pyramid
def allpairs_pyramid(f1, f2, levels):
    """CorrBlock.__init__ of the published RAFT in float64: corr[b, n1, (y2, x2)] = sum_c f1[b, c, n1] f2[b, c, n2] / sqrt(C), then
    avg_pool2d(2, 2) per level (an odd size drops its last row / column) -> list of [B, H W, H >> l, W >> l]"""
    B, C, H, W = f1.shape
    corr = torch.einsum("bcn,bcm->bnm", f1.double().reshape(B, C, H * W), f2.double().reshape(B, C, H * W)) / float(C) ** 0.5
    pyr = [corr.reshape(B, H * W, H, W)]
    for _ in range(levels - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


# ------------------------------------------------------------------------------------------------ CorrVolume
def _corr64(a, b, radius, stride):
    """(1/C) sum_c a[b, c, y, x] * b[b, c, y + dy stride, x + dx stride] in float64, zeros outside -> [B, (2r+1)^2, H, W]"""
    B, C, H, W = a.shape
    pad, D = radius * stride, 2 * radius + 1
    bp = F.pad(b, (pad, pad, pad, pad))
    out = a.new_empty(B, D * D, H, W)
    for i in range(D):
        for j in range(D):
            out[:, i * D + j] = (a * bp[:, :, i * stride:i * stride + H, j * stride:j * stride + W]).sum(1)
    return out / float(C)


def corr_volume_refs(cur, prev, radius, stride):
    """CorrVolume (oracle.ops.corr_volume) of float32 cur / prev [B, C, H, W] in float64, with the f16 hi/lo split of _split_exact.split_x
    (hi = fp16(x), lo = fp16(x - hi), subnormal lo halves kept) that corr_mfma.hip stages:
      true     the operator on the true operands
      y4       (1/C) sum (ch + cl)(ph + pl): all four split terms, what one K = 32 MFMA of corr_mfma.hip adds up
      y1       hi x hi only
      A        (1/C) sum (|ch| + |cl|)(|ph| + |pl|): the bound of every partial sum of the split kernel; 0 exactly where the displacement leaves the map
      A1       (1/C) sum |c| |p|: the same for the fp32 kernels
      d_last   the contribution of the last channel (true operands)
      d_lohi8  the cl x ph terms of the last 8 channels
    y4 - true is the split's own truncation, <= about 2^-21 A (each operand keeps 22 bits): an eighth of SPLIT_BAR = 2^-18.  The lo x lo
    term is smaller still (measured 0.005 - 0.023 of the bar at the shapes of test_kernel_refs_cpu.py): no test can tell a kernel that
    drops it from one that keeps it, and none asserts it."""
    from _split_exact import split_x
    assert cur.dtype == torch.float32 and prev.dtype == torch.float32 and cur.shape == prev.shape
    C = cur.shape[1]
    ch, cl = split_x(cur)
    ph, pl = split_x(prev)
    cd, pd = cur.double(), prev.double()
    lo8 = slice(max(0, C - 8), C)
    return dict(true=_corr64(cd, pd, radius, stride), y4=_corr64(ch + cl, ph + pl, radius, stride), y1=_corr64(ch, ph, radius, stride),
                A=_corr64(ch.abs() + cl.abs(), ph.abs() + pl.abs(), radius, stride), A1=_corr64(cd.abs(), pd.abs(), radius, stride),
                d_last=_corr64(cd[:, C - 1:], pd[:, C - 1:], radius, stride) / float(C),
                d_lohi8=_corr64(cl[:, lo8], ph[:, lo8], radius, stride) * (float(lo8.stop - lo8.start) / float(C)))
