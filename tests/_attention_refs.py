"""fp64 reference, bar, near-miss references, fp32 block-wise emulation and the row table of the attention core (csrc/attention.hip:
attention_cf_kernel<8|16|32|64>, route 0, and attention_cf_f16s_kernel<16|32|64>, route 1).  Shared by test_gpu_attention_routes.py (the
kernels against the reference) and test_attention_refs_cpu.py (the reference against itself).  A plain helper module: no tests live here.

The reference works per head, in float64, on the exact operands the kernel multiplies (heads_: [B, C, N] -> [B, heads, N, d]):

  qs = fp32(q * fp32(1 / sqrt(d)))                   one fp32 multiply, as the kernel does
  route 1: clamp qs, k, v to +-60000 (split_h8), then xh = fp16(x), xl = fp16(x - xh);   s3 = qh.kh + qh.kl + ql.kh over the head's d channels
  route 0: no split (xh = x, xl = 0);                                                     s3 = qs.k
  P   = softmax(s3) over the first nk_valid keys
  y   = P (vh + vl)
  A_s = (|qh| + |ql|) . (|kh| + |kl|)                per (query, key)
  A_o = P (|vh| + |vl|)
  e_s = SPLIT_BAR x max over the valid keys of A_s   per query
  bar = (2 e_s + SPLIT_BAR) x A_o

Derivation of the bar.  The kernel's output is o / l with o = sum_j w_j v_j, l = sum_j w_j and w_j = exp(s_j - m): a ratio of two sums over
the same weights, so the shift m (the running maximum, whatever order the blocks arrive in) cancels exactly and only the relative error of
each weight matters.  Let every computed weight be w_j (1 + eps_j), |eps_j| <= eps.  Then |o' - o| <= eps sum w_j |v_j| and |l' - l| <= eps l,
and to first order |o' / l' - o / l| <= eps (sum w_j |v_j|) / l + |o / l| eps <= 2 eps A_o, because |o / l| <= A_o = sum P_j |v_j|.

eps collects four things.
  (1) The accumulation error of the score.  The products of f16 halves are exact in fp32 (11 x 11 bits); each of the n MFMA instructions
      that accumulate into a score rounds once, each partial sum is at most A_s, so |s' - s3| <= (n + 1) u A_s with u = 2^-24.  n = 3 d / 16
      <= 12 on route 1 (three 32x32x16 f16 MFMAs per 16 channels), n = d / 2 <= 32 on route 0 (one 32x32x2 fp32 MFMA per two channels; its
      two products round like a two-term fp32 sum): n + 1 <= 33 is inside the 64 u = 2^-18 = SPLIT_BAR.  An absolute error delta of a score
      is a relative error exp(delta) - 1 ~ delta of its weight: this is e_s, and it is the only term that grows with the operands.
  (2) The rounding of s - m: u |s - m| <= 2 u max A_s, inside the same 64 u A_s (33 + 2 < 64).
  (3) expf: a few u relative, whatever A_s is.
  (4) The pl.vl term the f16-split kernel drops: P and V are each split to 22 bits, the dropped product is 2^-22 = 4 u relative to
      P |v|.
(3) and (4) do not scale with A_s; they are charged to the additive SPLIT_BAR, together with the accumulation of the PV product
(2 x 3 f16 MFMAs, or 16 fp32 MFMAs, per 32-key block, over Nk / 32 blocks) and the per-block rescales o *= alpha, l = l alpha + psum
(one rounding each per block).  Their certain bound grows with the block count (about 19 roundings per block on route 0); like the
2-D convolution tables (test_gpu_conv_f16s_routes.py, test_gpu_wino_stream_routes.py) the bar rests on these roundings being a random
walk, not a worst case: 19 Nk / 32 roundings of independent sign have a root-mean-square of sqrt(19 x 16) u ~ 17 u at Nk = 512, the
longest row, against 64 u.  SPLIT_BAR is the project's number; no constant is introduced here.

What the bar resolves is shown on the CPU (test_attention_refs_cpu.py), row by row, with a reference variant standing in for a broken
kernel (near-miss, key in refs["near"]):
  "qk_lo"    score from qh.kh only                              route-1 rows
  "v_lo"     PV from vh only                                    route-1 rows (weakest at long key sequences: Nk <= 512 here)
  "channel"  the last channel of every head left out of q.k     every row
  "mask-1"   nk_valid - 1 keys                                  masked rows
  "mask+1"   nk_valid + 1 keys (the first padded key, zero)     masked rows
  "heads"    b and h exchanged in the split of blockIdx.x       rows with B > 1
  "rescale"  o not multiplied by alpha (l is)                   the rows about the rescale path
  "clamp"    operands clamped at 65504 in place of 60000        the clamp row
and the fp32 block-wise emulation of each kernel (emulate: 32-key blocks, online max / sum / alpha, the three-term products, P split to
hi / lo, o x (1 / l)) stays below the bar on every row.  Its accumulation order is torch's on the CPU, not the MFMA's: it shows that the
bar leaves room for an fp32 implementation of this arithmetic, it says nothing about the GPU."""
import math
from collections import namedtuple

import torch

from _split_exact import SPLIT_BAR

NEG_INF = float("-inf")


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def heads_(x, heads):
    B, C, N = x.shape
    return x.reshape(B, heads, C // heads, N).permute(0, 1, 3, 2)


def unheads_(y):
    B, heads, N, d = y.shape
    return y.permute(0, 1, 3, 2).reshape(B, heads * d, N)


def scale_of(d):
    """(float)(1.0 / sqrt((double)d)), as the launcher computes it"""
    return torch.tensor(1.0 / math.sqrt(d), dtype=torch.float64).float()


def split(x, route, clamp=60000.0):
    """(hi, lo) in float64 of an fp32 tensor: route 1 split_h8 (clamp, fp16, fp16 of the exact remainder), route 0 the value itself"""
    assert x.dtype == torch.float32
    if route == 0:
        return x.double(), torch.zeros_like(x, dtype=torch.float64)
    c = x.clamp(-clamp, clamp)
    h = c.half()
    return h.double(), (c - h.float()).half().double()


def operands(q, k, v, heads, route, clamp=60000.0):
    """the six per-head operands [B, heads, N, d] in float64: qh, ql (of the scaled q), kh, kl, vh, vl"""
    d = q.shape[1] // heads
    qs = heads_(q, heads) * scale_of(d)
    assert qs.dtype == torch.float32
    return split(qs, route, clamp) + split(heads_(k, heads).contiguous(), route, clamp) + split(heads_(v, heads).contiguous(), route, clamp)


def _scores(qh, ql, kh, kl, nk, terms=3, drop_last=False):
    if drop_last:
        qh, ql, kh, kl = (t[..., :-1] for t in (qh, ql, kh, kl))
    kh, kl = kh[:, :, :nk], kl[:, :, :nk]
    s = qh @ kh.transpose(-1, -2)
    if terms == 3:
        s = s + qh @ kl.transpose(-1, -2) + ql @ kh.transpose(-1, -2)
    return s


def _attend(ops, nk, terms=3, v_lo=True, drop_last=False):
    qh, ql, kh, kl, vh, vl = ops
    P = torch.softmax(_scores(qh, ql, kh, kl, nk, terms, drop_last), -1)
    vv = (vh + vl if v_lo else vh)[:, :, :nk]
    return P @ vv, P


def _exchange(ops):
    """the operands the kernel would read with b = bh % B, h = bh / B in place of h = bh % heads, b = bh / heads"""
    B, heads = ops[0].shape[:2]
    bh = torch.arange(B * heads)
    ib, ih = bh % B, bh // B
    return tuple(t[ib, ih].reshape(t.shape) for t in ops)


def _no_rescale(ops, nk):
    """o accumulated block by block against the running maximum and never multiplied by alpha; l as it should be"""
    qh, ql, kh, kl, vh, vl = ops
    s = _scores(qh, ql, kh, kl, nk)
    m_final = s.max(-1, keepdim=True).values
    o = torch.zeros(s.shape[:-1] + (vh.shape[-1],), dtype=torch.float64)
    m_run = torch.full_like(m_final, NEG_INF)
    for kb in range(0, nk, 32):
        sb = s[..., kb:kb + 32]
        m_run = torch.maximum(m_run, sb.max(-1, keepdim=True).values)
        o = o + torch.exp(sb - m_run) @ (vh + vl)[:, :, kb:min(kb + 32, nk)]
    return o / torch.exp(s - m_final).sum(-1, keepdim=True)


def attention_refs(q, k, v, heads, nk_valid=None, route=1, claims=()):
    """q [B, C, Nq], k / v [B, C, Nk] fp32 on the CPU -> float64 [B, C, Nq] tensors: y (the reference), bar, true (fp64 attention of the true
    operands), and near[name] for every near-miss in `claims` (module docstring)"""
    assert q.dtype == k.dtype == v.dtype == torch.float32 and route in (0, 1)
    Nk = k.shape[2]
    nk = Nk if nk_valid is None else nk_valid
    d = q.shape[1] // heads
    ops = operands(q, k, v, heads, route)
    qh, ql, kh, kl, vh, vl = ops
    y, P = _attend(ops, nk)
    A_s = (qh.abs() + ql.abs()) @ (kh.abs() + kl.abs())[:, :, :nk].transpose(-1, -2)
    A_o = P @ (vh.abs() + vl.abs())[:, :, :nk]
    e_s = SPLIT_BAR * A_s.max(-1, keepdim=True).values
    bar = (2 * e_s + SPLIT_BAR) * A_o
    tq, tk, tv = heads_(q, heads).double() / math.sqrt(d), heads_(k, heads).double(), heads_(v, heads).double()
    true = torch.softmax(tq @ tk[:, :, :nk].transpose(-1, -2), -1) @ tv[:, :, :nk]
    near = {}
    for c in claims:
        if c == "qk_lo":
            near[c] = _attend(ops, nk, terms=1)[0]
        elif c == "v_lo":
            near[c] = _attend(ops, nk, v_lo=False)[0]
        elif c == "channel":
            near[c] = _attend(ops, nk, drop_last=True)[0]
        elif c == "mask-1":
            near[c] = _attend(ops, nk - 1)[0]
        elif c == "mask+1":
            near[c] = _attend(ops, nk + 1)[0]
        elif c == "heads":
            near[c] = _attend(_exchange(ops), nk)[0]
        elif c == "rescale":
            near[c] = _no_rescale(ops, nk)
        elif c == "clamp":
            near[c] = _attend(operands(q, k, v, heads, route, clamp=65504.0), nk)[0]
        else:
            raise KeyError(c)
    return dict(y=unheads_(y), bar=unheads_(bar), true=unheads_(true), near={c: unheads_(t) for c, t in near.items()})


def emulate(q, k, v, heads, nk_valid=None, route=1):
    """the kernel's arithmetic in fp32 on the CPU -> [B, C, Nq] float32: 32-key blocks, online max / sum / alpha, route 1 with the
    three-term products of the f16 halves and P split to hi / lo (pl.vl dropped), o x (1 / l) at the end"""
    f = torch.float32
    Nk = k.shape[2]
    nk = Nk if nk_valid is None else nk_valid
    qh, ql, kh, kl, vh, vl = (t.to(f) for t in operands(q, k, v, heads, route))
    o = torch.zeros(qh.shape, dtype=f)
    m_run = torch.full(qh.shape[:-1] + (1,), NEG_INF, dtype=f)
    l_run = torch.zeros_like(m_run)
    for kb in range(0, Nk, 32):
        bh_, bl_ = kh[:, :, kb:kb + 32].transpose(-1, -2), kl[:, :, kb:kb + 32].transpose(-1, -2)
        s = qh @ bh_ if route == 0 else (qh @ bl_ + ql @ bh_) + qh @ bh_
        if kb + 32 > nk:
            s[..., nk - kb:] = NEG_INF
        m_new = torch.maximum(m_run, s.max(-1, keepdim=True).values)
        alpha = torch.exp(m_run - m_new)
        m_run = m_new
        p = torch.exp(s - m_new)
        l_run = l_run * alpha + p.sum(-1, keepdim=True)
        o = o * alpha
        if route == 0:
            o = o + p @ vh[:, :, kb:kb + 32]
        else:
            ph = p.half()
            pl = (p - ph.float()).half().float()
            ph = ph.float()
            o = ((o + ph @ vl[:, :, kb:kb + 32]) + pl @ vh[:, :, kb:kb + 32]) + ph @ vh[:, :, kb:kb + 32]
    assert o.dtype == f and l_run.dtype == f
    return unheads_(o * (1.0 / l_run))


# =========================================================================================================================== the rows
# route: the kernel the row is for (0 attention_cf_kernel<d>, 1 attention_cf_f16s_kernel<d>).  misv: V four bytes off a 16-byte boundary
# (what sends d >= 16 to route 0).  kind: how the inputs are made (row_inputs).  unit: O(1) operands, the standing 2e-5 applies.
Row = namedtuple("Row", "name route d B heads Nq Nk nk_valid kind seed misv unit claims")


def _row(name, route, d, B, heads, Nq, Nk, nk_valid=None, kind="randn", seed=0, unit=True, drop=(), extra=()):
    """the near-misses a row answers for: one channel everywhere, the lo halves on route 1, the b / h exchange where B > 1, the mask
    boundary on both sides where keys are padded; `drop` and `extra` adjust that, with the reason in the comment of the group"""
    nk = Nk if nk_valid is None else nk_valid
    claims = ["channel"] + (["qk_lo", "v_lo"] if route == 1 else []) + (["heads"] if B > 1 else [])
    if nk < Nk:
        claims += ["mask+1"] + (["mask-1"] if nk > 1 else [])
    if nk == 1:                                          # one key: the softmax is 1 whatever the score is
        drop = tuple(drop) + ("channel", "qk_lo")
    claims = tuple(c for c in claims if c not in drop) + tuple(extra)
    return Row(name, route, d, B, heads, Nq, Nk, nk, kind, seed, route == 0 and d >= 16, unit, claims)


KERNELS = [(1, 16), (1, 32), (1, 64), (0, 8), (0, 16), (0, 32), (0, 64)]
KNAME = lambda route, d: ("f16s" if route else "fp32") + "-d%d" % d          # noqa: E731

# two query blocks, the second with one active wave of four; three key blocks, so both LDS buffers of the f16-split kernel are reused
BLOCK_ROWS = [_row("blocks-%s" % KNAME(r, d), r, d, 2, 3, 160, 96, seed=9100 + 10 * r + d) for r, d in KERNELS]

# every residue of the masked key index (r & 3) + 8 (r >> 2) + 4 half that a boundary can fall on: both halves, both 4-runs, the 8-strides
MASK_KERNELS = [(1, 16), (1, 64), (0, 8), (0, 32)]
MASK_NK = [33, 36, 37, 40, 44, 45, 48, 49, 61, 63, 64]
MASK_ROWS = [_row("mask-%s-nk%d" % (KNAME(r, d), nk), r, d, 2, 3, 32, 64, nk, seed=9200 + 100 * r + d + nk) for r, d in MASK_KERNELS for nk in MASK_NK] + \
            [_row("mask-%s-one-key" % KNAME(r, d), r, d, 2, 3, 32, 32, 1, seed=9300 + 10 * r + d) for r, d in MASK_KERNELS]

# q, k, v as channel slices of fused projection buffers (test_gpu_attention_routes.py runs each in three layouts)
STRIDE_ROWS = [_row("strides-%s" % KNAME(r, d), r, d, 2, 3, 64, 64, seed=9400 + d) for r, d in ((0, 8), (1, 32))]

# the rescale path, deterministic: "asc" every 32-key block's maximum score exceeds the previous block's for every query (alpha < 1 at every
# block), "desc" the reverse (alpha == 1 after the first block).  Their lo halves are small by construction (amplitude 0.25 beside an exact
# channel 0), so the lo near-misses are not theirs; "rescale" is asc's.  "q8": unit normals with q x 8, one key dominates each query and
# the running maximum moves often.  A leaked padded key or one dropped lo half is not resolvable against a dominating key, so these rows claim
# neither the mask nor the lo near-misses: they are about alpha.
LO = ("qk_lo", "v_lo")
RESCALE_ROWS = []
for r, d in ((1, 64), (0, 8)):
    RESCALE_ROWS += [_row("rescale-%s-asc" % KNAME(r, d), r, d, 2, 3, 32, 128, kind="asc", seed=9500 + d, drop=LO, extra=("rescale",)),
                     _row("rescale-%s-desc" % KNAME(r, d), r, d, 2, 3, 32, 128, kind="desc", seed=9500 + d, drop=LO),
                     _row("rescale-%s-q8" % KNAME(r, d), r, d, 2, 3, 32, 128, kind="q8", seed=9510 + d, unit=False, drop=LO, extra=("rescale",))]

# sixteen key blocks (B = 1: the b / h exchange is the identity there, not claimed)
LONG_ROWS = [_row("long-%s" % KNAME(r, d), r, d, 1, 2, 32, 512, seed=9600 + d) for r, d in ((1, 64), (0, 8))]

# a few |k| and |v| above the f16 range: split_h8 clamps to +-60000.  The clamped keys dominate their queries completely, so only the
# clamp itself, one channel and the b / h exchange are claimed
CLAMP_ROWS = [_row("clamp-f16s-d32", 1, 32, 2, 3, 32, 64, kind="clamp", seed=9700, unit=False, drop=LO, extra=("clamp",))]

# ops.attention_cf on ragged token counts: the two masked kernels the ragged case of test_gpu_ops.py never reaches.  The reference is
# taken on the zero-padded tensors the wrapper builds
WRAPPER_ROWS = [_row("wrapper-%s-%dx%d" % (KNAME(r, d), Nq, Nk), r, d, 2, 3, (Nq + 31) // 32 * 32, (Nk + 31) // 32 * 32, Nk, kind="wrapper:%d" % Nq,
                     seed=9800 + d + Nq + Nk)
                for r, d in ((0, 8), (1, 16)) for Nq, Nk in ((45, 70), (33, 97), (64, 40), (1, 1))]

ROWS = BLOCK_ROWS + MASK_ROWS + STRIDE_ROWS + RESCALE_ROWS + LONG_ROWS + CLAMP_ROWS + WRAPPER_ROWS


def row_inputs(row):
    """(q, k, v) fp32 on the CPU, [B, heads d, Nq | Nk]; keys from nk_valid on are zero (the padding of ops.attention_cf)"""
    B, C, d = row.B, row.heads * row.d, row.d
    q, k, v = randn(B, C, row.Nq, seed=row.seed), randn(B, C, row.Nk, seed=row.seed + 1), randn(B, C, row.Nk, seed=row.seed + 2)
    if row.kind in ("asc", "desc"):
        q, k = 0.25 * q, 0.25 * k
        level = torch.arange(row.Nk // 32, dtype=torch.float32).repeat_interleave(32) - (row.Nk // 32 - 1) / 2.0      # -1.5 .. 1.5 by block
        if row.kind == "desc":
            level = -level
        qv, kv = q.view(B, row.heads, d, row.Nq), k.view(B, row.heads, d, row.Nk)
        qv[:, :, 0] = 2.0
        kv[:, :, 0] = level
        s = heads_(q, row.heads).double() @ heads_(k, row.heads).double().transpose(-1, -2) / math.sqrt(d)
        bmax = s.view(B, row.heads, row.Nq, row.Nk // 32, 32).max(-1).values
        step = bmax[..., 1:] - bmax[..., :-1]
        assert bool((step > 0.05).all() if row.kind == "asc" else (step < -0.05).all()), "block maxima are not ordered for every query"
    elif row.kind == "q8":
        q = 8.0 * q
    elif row.kind == "clamp":
        kv, vv = k.view(B, row.heads, d, row.Nk), v.view(B, row.heads, d, row.Nk)
        kv[0, 0, 3, 5], kv[1, 2, 31, 40], kv[1, 1, 0, 63] = 7e4, -1e5, 65520.0
        vv[0, 1, 7, 2], vv[1, 0, 30, 33], vv[0, 2, 16, 63], vv[1, 2, 1, 40] = 7e4, -3e5, 65520.0, 1e6
    elif row.kind.startswith("wrapper"):
        q[:, :, int(row.kind.split(":")[1]):] = 0.0
    if row.nk_valid < row.Nk:
        k[:, :, row.nk_valid:] = 0.0
        v[:, :, row.nk_valid:] = 0.0
    return q, k, v


def garbage_padding(row, k, v):
    """copies of k, v with finite garbage in the padded keys: K random, V = 1000"""
    k, v = k.clone(), v.clone()
    n = row.Nk - row.nk_valid
    k[:, :, row.nk_valid:] = 3.0 * randn(k.shape[0], k.shape[1], n, seed=row.seed + 7)
    v[:, :, row.nk_valid:] = 1000.0
    return k, v


def row_refs(row):
    q, k, v = row_inputs(row)
    return (q, k, v), attention_refs(q, k, v, row.heads, row.nk_valid, row.route, row.claims)


def worst_ratio(got, want, bar):
    """max |got - want| / bar; an element with bar == 0 must be met exactly; NaN if anything is not finite"""
    diff = (got.double() - want).abs()
    r = torch.where(bar > 0, diff / bar, torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())
