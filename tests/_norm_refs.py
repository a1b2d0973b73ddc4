"""fp64 references, bars and row tables of the normalisation kernels (csrc/norm.hip), shared by test_gpu_norm_routes.py (the kernels against
them), test_norm_refs_cpu.py (the references against torch, fp32 emulations of the kernels against the bars, the near-misses against the
bars) and test_abi_and_host.py (the plan of every row from cf_group_norm_route).  A plain helper module: no tests live here.

u = 2^-24 throughout; every reference is formed in float64 from the stored fp32 operands; eps is double(float32(1e-5)), what the kernels
widen their float argument to.

Statistics (gn_stats_wave_kernel, gn_stats_block_kernel): S = sum x, SS = sum x^2 per (sample, group) slab of L = (C / groups) HW values.
  wave   every value is widened first and accumulated in fp64: 64 lanes with L / 64 adds each and a 6-step butterfly, so a chain of at most
         L / 64 + 6 roundings of 2^-53: for L <= 2^21 under 2^-37 of (sum |x|, sum x^2).  Bar 2^-36 (sum |x|, sum x^2).
  block  a float4 is reduced in fp32 before it is widened: x + y and z + w (one rounding u |x + y| each), x x + y y and z z + w w (two
         roundings with a fused multiply-add, three without: at most 2 u (x^2 + y^2)); everything after that is fp64.  First order:
         |dS| <= u sum |x|, |dSS| <= 2 u sum x^2 = 2^-23 sum x^2.  Bars 2^-23 sum |x| and 2^-22 sum x^2, twice that.  Relative to the
         variance this is 2^-22 (mean^2 + var) / var: invisible at mean / std = 0.5, 1e-3 at mean / std = 64 -- in the worst case; the
         roundings are independent and the measured figure is far smaller (profiles/norm_route_table.md).

Apply (gn_apply_kernel, gn_apply_small_kernel, layer_norm_cf_kernel): y = (x - mean) rstd g + b with mean = S / L and var = SS / L - mean^2
from the fp64 sums the kernel is given (or forms itself, LayerNorm).  The kernel rounds mean and rstd to fp32 (u |mean|, u rstd) and runs
x - mean, * rstd, * g, + b in fp32 (one rounding each, the last two possibly fused).  First order:
  |dy| <= u (|mean| + 5 |x - mean|) rstd |g| + u |b|  <=  5 u M,   M = (|x| + |mean|) rstd |g| + |b|.
Bar 2^-21 M = 8 u M.  A residual r' = (r - rm) ra + rb has Mr = (|r| + |rm|) |ra| + |rb| (a plain residual: rm = 0, ra = 1, rb = 0, Mr = |r|),
and with an activation or a residual the bar is 1.13 * 2^-21 (M + Mr) + E_act(v) + 2^-23 |ref|, v the fp64 pre-activation: 1.13 is GELU's
largest slope (every other activation here has slope <= 1), 2^-23 |ref| the roundings behind the activation, and
  E_act: none, relu, lrelu 0;  gelu |v| / 2 (1.5e-7 + 16 u): the erf bound of Abramowitz & Stegun 7.1.26 as common.h states it, and the fp32
         Horner chain, rcp and exp2 of gelu_as;  tanh, sigmoid 2^-21 (library functions, a few ulp of a value <= 1).
LeakyReLU's slope is double(float32(0.01)), the kernel's constant.

gn_coef_kernel: {mean, scale, shift}: |mean_f - mean| <= u |mean| (one rounding), scale within 2^-22 of rstd gamma (two roundings), shift
bitwise beta.

norm_head_1x1_kernel: ref = bias + sum_c w lrelu((x - m) sc + sh) of the fp32 coefficient tensor as given.  Each term carries three
roundings and the slope's (<= 4 u of |x - m| |sc| + |sh|), then C fused multiply-adds each rounding a partial sum bounded by
A = |bias| + sum_c |w| (|x - m| |sc| + |sh|).  Bar (C + 4) u A.

Near-misses (reference variants one slip away, which the bar must reject; asserted on the CPU, row by row): statistics without the slab's
last element, without the last partial sweep, without one float4; variance over L - 1; the neighbouring slab's statistics; the residual
added on the other side of the activation; eps / 10 and eps = 0 on small-variance data; LayerNorm over C - 1 and without the last channel;
the head without its last channel and with slope 0; the tanh form of GELU."""
import collections
import math

import numpy as np
import torch

U = 2.0 ** -24
EPS = float(np.float32(1e-5))
SLOPE = float(np.float32(0.01))
ACTS = ("none", "gelu", "relu", "lrelu", "tanh", "sigmoid")


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def make_data(kind, shape, seed):
    z = randn(*shape, seed=seed)
    return {"std": 3.0 * z + 1.5, "offset": 64.0 + z, "offset2": 64.0 + 2.0 * z, "smallvar": 0.2 + 0.01 * z, "zscore": 50.0 * z + 300.0}[kind].float()


def ratio(got, ref, bar):
    """worst |got - ref| / bar; an exact hit under a zero bar counts 0, anything else there (and every NaN) inf"""
    err = (got.double() - ref).abs()
    r = torch.where(bar > 0, err / bar, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
# B, C, HW, groups, view (x one float into a NaN-fenced buffer), data, expected plan[0:3] = (kernel, segs, blocks), near-misses
StatsRow = collections.namedtuple("StatsRow", "name B C HW groups view data plan near")
STATS_ROWS = (
    StatsRow("wave-at-the-line", 2, 8, 2048, 4, False, "std", (0, 0, 2), ("last",)),
    StatsRow("block-segs1-lone-float4", 3, 1, 4100, 1, False, "std", (1, 1, 3), ("last", "float4-1024")),
    StatsRow("wave-L105-9slabs", 3, 9, 35, 3, False, "std", (0, 0, 3), ("last",)),
    StatsRow("wave-L35-9slabs", 3, 3, 35, 3, False, "std", (0, 0, 3), ("last",)),
    StatsRow("wave-odd-L4099", 2, 1, 4099, 1, False, "std", (0, 0, 1), ("last",)),
    StatsRow("block-segs4-ragged", 1, 1, 24580, 1, False, "std", (1, 4, 4), ("last",)),
    StatsRow("block-clamp64", 1, 2, 1052672, 2, False, "std", (1, 64, 128), ("sweep",)),
    StatsRow("wave-view-L4096", 2, 4, 2048, 2, True, "std", (0, 0, 1), ("last",)),
    StatsRow("wave-view-L8192", 2, 4, 4096, 2, True, "std", (0, 0, 1), ("last",)),          # misaligned alone keeps it off the block kernel
    StatsRow("offset-wave", 2, 16, 512, 8, False, "offset", (0, 0, 4), ("last",)),
    StatsRow("offset-block", 2, 16, 4096, 8, False, "offset", (1, 1, 16), ("last",)),
)


def slab_sums(x, groups):
    v = x.double().reshape(x.shape[0], groups, -1)
    return v.sum(-1), (v * v).sum(-1), v.abs().sum(-1)


def host_ws(x, groups):
    """the statistics workspace [B, groups, 2] in fp64, formed on the host"""
    S, SS, _ = slab_sums(x, groups)
    return torch.stack([S, SS], -1)


def stats_case(row):
    """x [B, C, HW] (the last element of every slab is 1.5), the fp64 sums, the bars, and the near-miss sums by name"""
    x = make_data(row.data, (row.B, row.C, row.HW), seed=100 + STATS_ROWS.index(row))
    xs = x.view(row.B, row.groups, -1)
    xs[:, :, -1] = 1.5
    S, SS, SA = slab_sums(x, row.groups)
    block = row.plan[0] == 1
    bars = torch.stack([SA * 2.0 ** (-23 if block else -36), SS * 2.0 ** (-22 if block else -36)], -1)
    ref = torch.stack([S, SS], -1)
    L = xs.shape[-1]
    cut = {"last": slice(L - 1, L), "float4-1024": slice(4096, 4100), "sweep": slice(L - 4 * ((L // 4) % (row.plan[1] * 256 if block else 1)), L)}
    near = {}
    for name in row.near:
        d = xs[:, :, cut[name]].double()
        assert d.shape[-1] > 0
        near[name] = ref - torch.stack([d.sum(-1), (d * d).sum(-1)], -1)
    return dict(x=x, ref=ref, bar=bars, near=near, L=L)


def emulate_block_stats(x, groups):
    """gn_stats_block_kernel's sums: the pair sums of a float4 in fp32 (no fused multiply-add: one rounding more than the kernel), then fp64"""
    v = x.reshape(x.shape[0], groups, -1, 4)
    a, b = v[..., 0] + v[..., 1], v[..., 2] + v[..., 3]
    qa, qb = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1], v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3]
    return torch.stack([(a.double() + b.double()).sum(-1), (qa.double() + qb.double()).sum(-1)], -1)


def variance_of(ws, L):
    mean = ws[..., 0] / L
    return ws[..., 1] / L - mean * mean


# ---- activations -----------------------------------------------------------------------------------------------------------------------
def act64(v, act):
    if act == "gelu":
        return 0.5 * v * (1.0 + torch.special.erf(v / math.sqrt(2.0)))
    if act == "relu":
        return torch.where(v < 0, torch.zeros_like(v), v)
    if act == "lrelu":
        return torch.where(v > 0, v, SLOPE * v)
    if act == "tanh":
        return torch.tanh(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    assert act in (None, "none")
    return v


def gelu_tanh64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def e_act(v, act):
    if act == "gelu":
        return v.abs() / 2 * (1.5e-7 + 16 * U)
    if act in ("tanh", "sigmoid"):
        return torch.full_like(v, 2.0 ** -21)
    return torch.zeros_like(v)


def gelu_as_f32(v):
    """common.h's gelu_as, operation by operation in fp32 (a true reciprocal and exp2 for the hardware's, no fused multiply-adds)"""
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    z = v.abs() * f(0.70710678118654752440)
    t = 1.0 / (f(0.3275911) * z + 1.0)
    poly = t * (t * (t * (t * (t * f(1.061405429) + f(-1.453152027)) + f(1.421413741)) + f(-0.284496736)) + f(0.254829592))
    e = torch.exp2(-z * z * f(1.44269504088896340736))
    return 0.5 * v * (1.0 + torch.copysign(1.0 - poly * e, v))


def act_f32(v, act):
    assert v.dtype == torch.float32
    if act == "gelu":
        return gelu_as_f32(v)
    if act == "relu":
        return torch.where(v < 0, torch.zeros_like(v), v)
    if act == "lrelu":
        return torch.where(v > 0, v, torch.tensor(0.01, dtype=torch.float32) * v)
    if act == "tanh":
        return torch.tanh(v)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def sweep_inputs():
    """the two input vectors of the activation sweep: the dense interval, then the logarithmic tails and the special finite values"""
    dense = torch.linspace(-12.0, 12.0, 2 ** 21 + 1, dtype=torch.float64).float()
    tail = torch.logspace(-30.0, 1.2, 20001, dtype=torch.float64).float()
    tiny = float(np.finfo(np.float32).tiny)
    special = torch.tensor([0.0, -0.0, tiny, -tiny, tiny / 8, -tiny / 8, 65504.0, -65504.0, 1e30, -1e30], dtype=torch.float32)
    return dense, torch.cat([tail, -tail, special])


def sweep_refs(v32, act):
    """(ref, bar) of act(v) in fp64; lrelu's negative side is the exact product of two fp32 values rounded once, as an fp32 multiply gives it"""
    v = v32.double()
    ref = act64(v, act)
    bar = e_act(v, act) + (U * ref.abs() if act == "gelu" else 0.0)
    if act == "lrelu":
        ref = ref.float().double()
    return ref, bar


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
def moments(ws, L, eps, bessel=False):
    mean = ws[..., 0] / L
    var = (ws[..., 1] / L - mean * mean).clamp_min(0.0)
    if bessel:
        var = var * L / (L - 1)
    return mean, 1.0 / torch.sqrt(var + eps)


def _chan(t, C, groups):
    """[B, groups] -> [B, C, 1]"""
    return t.repeat_interleave(C // groups, dim=1)[..., None]


def _affine(p, C, fill):
    return torch.full((1, C, 1), fill, dtype=torch.float64) if p is None else p.double().view(1, C, 1)


def apply_refs(x, ws, gamma, beta, groups, eps=EPS, act="none", res=None, res_mode=None, res_norm=None, bessel=False):
    """x, res [B, C, HW] fp32; ws [B, groups, 2] fp64; res_norm = (ws_r, gamma_r, beta_r) -> (ref, bar) in fp64"""
    B, C, HW = x.shape
    L = C // groups * HW
    mean, rstd = (_chan(t, C, groups) for t in moments(ws.view(B, groups, 2), L, eps, bessel))
    g, b = _affine(gamma, C, 1.0), _affine(beta, C, 0.0)
    xd = x.double()
    y = (xd - mean) * rstd * g + b
    M = (xd.abs() + mean.abs()) * rstd * g.abs() + b.abs()
    r = Mr = torch.zeros_like(y)
    if res is not None and res_mode in ("before_act", "after_act"):
        rd = res.double()
        if res_norm is not None:
            rm, rr = (_chan(t, C, groups) for t in moments(res_norm[0].view(B, groups, 2), L, eps))
            ra, rb = rr * _affine(res_norm[1], C, 1.0), _affine(res_norm[2], C, 0.0)
            r, Mr = (rd - rm) * ra + rb, (rd.abs() + rm.abs()) * ra.abs() + rb.abs()
        else:
            r, Mr = rd, rd.abs()
    v = y + r if res_mode == "before_act" else y
    ref = act64(v, act) + (r if res_mode == "after_act" else 0.0)
    if act in (None, "none") and res_mode is None:
        return ref, 2.0 ** -21 * M
    return ref, 1.13 * 2.0 ** -21 * (M + Mr) + e_act(v, act) + 2.0 ** -23 * ref.abs()


def emulate_apply(x, ws, gamma, beta, groups, eps=EPS, act="none", res=None, res_mode=None, res_norm=None):
    """the kernels' expression in fp32: mean and rstd rounded from the fp64 sums, then one fp32 operation at a time"""
    B, C, HW = x.shape
    L = C // groups * HW
    f = lambda p, fill: torch.full((1, C, 1), fill) if p is None else p.float().view(1, C, 1)
    mean, rstd = (_chan(t, C, groups).float() for t in moments(ws.view(B, groups, 2), L, eps))
    y = (x - mean) * rstd * f(gamma, 1.0) + f(beta, 0.0)
    r = None
    if res is not None and res_mode in ("before_act", "after_act"):
        r = res
        if res_norm is not None:
            rm, rr = (_chan(t, C, groups).float() for t in moments(res_norm[0].view(B, groups, 2), L, eps))
            r = (res - rm) * (rr * f(res_norm[1], 1.0)) + f(res_norm[2], 0.0)
    if res_mode == "before_act":
        y = y + r
    y = act_f32(y, act)
    if res_mode == "after_act":
        y = y + r
    return y


# B, C, HW, groups; which operand is a misaligned view ("", "x", "res"); in place; data; the whole plan8; extra forms
ApplyRow = collections.namedtuple("ApplyRow", "name B C HW groups view inplace data plan extra")
APPLY_ROWS = (
    ApplyRow("small-vec-one-short-block", 3, 8, 36, 4, "", False, "std", (0, 0, 3, 0, 1, 113, 1, 24), True),
    ApplyRow("small-ppb4-last3", 3, 9, 1024, 3, "", False, "std", (0, 0, 3, 0, 1, 4, 7, 3), False),
    ApplyRow("small-ppb-clamp512", 2, 600, 4, 8, "", False, "std", (0, 0, 4, 0, 1, 512, 3, 176), False),
    ApplyRow("small-hw1", 3, 700, 1, 7, "", False, "std", (0, 0, 6, 0, 0, 512, 5, 52), False),
    ApplyRow("small-scalar-hw3", 2, 8, 3, 4, "", False, "std", (0, 0, 2, 0, 0, 512, 1, 16), False),
    ApplyRow("small-scalar-hw35", 3, 8, 35, 8, "", False, "std", (0, 0, 6, 0, 0, 117, 1, 24), False),
    ApplyRow("small-scalar-hw2047", 2, 4, 2047, 2, "", False, "std", (0, 0, 1, 0, 0, 2, 4, 2), False),
    ApplyRow("small-vec-hw2044", 2, 4, 2044, 2, "", False, "std", (0, 0, 1, 0, 1, 2, 4, 2), False),
    ApplyRow("large-vec-asegs1", 2, 16, 2048, 8, "", False, "std", (0, 0, 4, 1, 1, 1, 32, 0), True),
    ApplyRow("large-vec-asegs2", 2, 4, 4100, 2, "", False, "std", (1, 2, 8, 1, 1, 2, 16, 0), False),
    ApplyRow("large-scalar-asegs3", 2, 8, 2115, 4, "", False, "std", (0, 0, 2, 1, 0, 3, 48, 0), False),
    ApplyRow("large-scalar-x-view", 2, 16, 2048, 8, "x", False, "std", (0, 0, 4, 1, 0, 2, 64, 0), False),
    ApplyRow("large-scalar-res-view", 2, 16, 2048, 8, "res", False, "std", (0, 0, 4, 1, 0, 2, 64, 0), False),
    ApplyRow("large-vec-in-place", 2, 16, 2048, 8, "", True, "std", (0, 0, 4, 1, 1, 1, 32, 0), False),
    ApplyRow("small-offset", 3, 8, 36, 4, "", False, "offset", (0, 0, 3, 0, 1, 113, 1, 24), False),
    ApplyRow("large-offset", 2, 16, 2048, 8, "", False, "offset", (0, 0, 4, 1, 1, 1, 32, 0), False),
    ApplyRow("small-smallvar", 3, 8, 36, 4, "", False, "smallvar", (0, 0, 3, 0, 1, 113, 1, 24), False),
    ApplyRow("large-smallvar", 2, 16, 2048, 8, "", False, "smallvar", (0, 0, 4, 1, 1, 1, 32, 0), False),
)
# name -> (act, residual: None / "plain" / "norm", res_mode, null affine)
FORMS = collections.OrderedDict((
    ("plain", ("none", None, None, False)),
    ("gelu+res-after", ("gelu", "plain", "after_act", False)),
    ("gelu+res-before", ("gelu", "plain", "before_act", False)),
    ("lrelu", ("lrelu", None, None, False)),
    ("gelu+resnorm-after", ("gelu", "norm", "after_act", False)),
    ("gelu+resnorm-before", ("gelu", "norm", "before_act", False)),
))
EXTRA_FORMS = collections.OrderedDict((
    ("relu", ("relu", None, None, False)),
    ("tanh", ("tanh", None, None, False)),
    ("sigmoid", ("sigmoid", None, None, False)),
    ("null-affine", ("none", None, None, True)),
))
OTHER_MODE = {"after_act": "before_act", "before_act": "after_act"}


def forms_of(row):
    names = list(FORMS) + (list(EXTRA_FORMS) if row.extra else [])
    if row.view == "res" or row.inplace:
        names = ["plain", "gelu+res-after", "gelu+res-before"] if row.inplace else ["gelu+res-after", "gelu+res-before", "gelu+resnorm-after"]
    return names


def apply_inputs(row):
    """x, res [B, C, HW], per-channel parameters of both norms and both host workspaces; one set per row, shared by its forms"""
    i = APPLY_ROWS.index(row)
    shape = (row.B, row.C, row.HW)
    x, res = make_data(row.data, shape, seed=200 + i), make_data("std", shape, seed=300 + i)
    p = randn(4, row.C, seed=400 + i)
    return dict(x=x, res=res, gamma=1.0 + 0.5 * p[0], beta=p[1], gamma_r=1.0 + 0.5 * p[2], beta_r=p[3], ws=host_ws(x, row.groups),
                ws_r=host_ws(res, row.groups))


def form_kwargs(inp, form):
    """the keyword arguments of apply_refs / emulate_apply / ops.group_norm_apply (tensors on the CPU) for one form"""
    act, resk, mode, null = (FORMS.get(form) or EXTRA_FORMS[form])
    kw = dict(gamma=None if null else inp["gamma"], beta=None if null else inp["beta"], act=act)
    if resk:
        kw.update(res=inp["res"], res_mode=mode)
        if resk == "norm":
            kw["res_norm"] = (inp["ws_r"], inp["gamma_r"], inp["beta_r"])
    return kw


def apply_near_misses(row, inp, form, ref, bar):
    """name -> multiple of the bar by which a reference one slip away misses the true one"""
    kw = form_kwargs(inp, form)
    L = row.C // row.groups * row.HW
    out = {}
    nb = torch.roll(inp["ws"].view(-1, 2), 1, 0).view(row.B, row.groups, 2)
    out["neighbour-slab"] = ratio(apply_refs(inp["x"], nb, groups=row.groups, **kw)[0], ref, bar)
    if L <= 8192:
        out["L-1"] = ratio(apply_refs(inp["x"], inp["ws"], groups=row.groups, bessel=True, **kw)[0], ref, bar)
    if kw.get("res_mode"):
        out["other-mode"] = ratio(apply_refs(inp["x"], inp["ws"], groups=row.groups, **dict(kw, res_mode=OTHER_MODE[kw["res_mode"]]))[0], ref, bar)
    if row.data == "smallvar":
        out["eps/10"] = ratio(apply_refs(inp["x"], inp["ws"], groups=row.groups, eps=EPS / 10, **kw)[0], ref, bar)
        out["eps=0"] = ratio(apply_refs(inp["x"], inp["ws"], groups=row.groups, eps=0.0, **kw)[0], ref, bar)
    return out


CONST_A = float(np.float32(100.1))


def constant_slab_inputs(row):
    """the row's inputs with slab 0 constant at float32(100.1) and slab 1 at 0; their workspace entries are L v and L v^2 exactly rounded,
    so that mean is v to 2^-52 and rounds back to v: x - fp32(mean) is exactly 0 and the output bitwise beta[c]"""
    inp = apply_inputs(row)
    L = row.C // row.groups * row.HW
    xs = inp["x"].view(row.B * row.groups, L)
    xs[0], xs[1] = CONST_A, 0.0
    ws = host_ws(inp["x"], row.groups)
    ws.view(-1, 2)[0] = torch.tensor([L * CONST_A, L * (CONST_A * CONST_A)], dtype=torch.float64)
    ws.view(-1, 2)[1] = 0.0
    inp["ws"] = ws
    return inp


def propagate_stats_bar(x, ws, gamma, groups, eps, block):
    """what the statistics bar of the route taken adds to the apply bar of a composed cf_group_norm: the mean through rstd |g| dmean, the
    variance through |x - mean| rstd |g| dvar / (2 (var + eps)), dvar <= dSS / L + 2 |mean| dmean"""
    B, C, HW = x.shape
    L = C // groups * HW
    _, SS, SA = slab_sums(x, groups)
    dS, dSS = SA * 2.0 ** (-23 if block else -36), SS * 2.0 ** (-22 if block else -36)
    mean, rstd = moments(ws, L, eps)
    dmean, dvar = dS / L, dSS / L + 2 * mean.abs() * dS / L
    g = _affine(gamma, C, 1.0).abs()
    c = lambda t: _chan(t, C, groups)
    return c(rstd) * g * c(dmean) + (x.double() - c(mean)).abs() * c(rstd) ** 3 * g * c(dvar) / 2


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
LnRow = collections.namedtuple("LnRow", "name B C N view inplace data")
LN_ROWS = (
    LnRow("registers-at-the-line", 2, 256, 70, False, False, "std"),
    LnRow("reread-at-the-line", 2, 257, 70, False, False, "std"),
    LnRow("one-channel", 3, 1, 65, False, False, "std"),
    LnRow("one-channel-per-wave", 2, 8, 64, False, False, "std"),
    LnRow("ninth-channel", 2, 9, 33, False, False, "std"),
    LnRow("one-token", 1, 264, 1, False, False, "std"),
    LnRow("straddles-samples", 5, 40, 13, False, False, "std"),
    LnRow("offset-registers", 2, 256, 70, False, False, "offset2"),
    LnRow("offset-reread", 2, 512, 70, False, False, "offset2"),
    LnRow("reread-view", 2, 257, 70, True, False, "std"),
    LnRow("reread-in-place", 2, 512, 70, False, True, "std"),
    LnRow("registers-in-place", 2, 64, 70, False, True, "std"),
)


def ln_inputs(row):
    i = LN_ROWS.index(row)
    p = randn(2, row.C, seed=600 + i)
    return dict(x=make_data(row.data, (row.B, row.C, row.N), seed=500 + i), gamma=1.0 + 0.5 * p[0], beta=p[1])


def ln_refs(x, gamma, beta, eps=EPS, bessel=False, drop_last=False):
    xd = x.double()
    xs = xd[:, :-1] if drop_last else xd
    n = xs.shape[1]
    mean = xs.sum(1, keepdim=True) / n
    var = ((xs * xs).sum(1, keepdim=True) / n - mean * mean).clamp_min(0.0)
    if bessel:
        var = var * n / (n - 1)
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = gamma.double().view(1, -1, 1), beta.double().view(1, -1, 1)
    return (xd - mean) * rstd * g + b, 2.0 ** -21 * ((xd.abs() + mean.abs()) * rstd * g.abs() + b.abs())


def emulate_ln(x, gamma, beta, eps=EPS):
    xd = x.double()
    C = x.shape[1]
    mean = xd.sum(1, keepdim=True) / C
    var = ((xd * xd).sum(1, keepdim=True) / C - mean * mean).clamp_min(0.0)
    return (x - mean.float()) * (1.0 / torch.sqrt(var + eps)).float() * gamma.float().view(1, -1, 1) + beta.float().view(1, -1, 1)


# ---- gn_coef ---------------------------------------------------------------------------------------------------------------------------
CoefRow = collections.namedtuple("CoefRow", "name B C HW groups null const")
COEF_ROWS = (
    CoefRow("one-block", 2, 16, 100, 8, False, False),
    CoefRow("instance-odd", 3, 5, 7, 5, False, False),
    CoefRow("second-block", 1, 300, 9, 1, False, False),
    CoefRow("second-block-groups3", 2, 129, 4, 3, False, False),
    CoefRow("null-affine", 2, 16, 100, 8, True, False),
    CoefRow("constant-slab", 2, 16, 100, 8, False, True),
)


def coef_inputs(row):
    i = COEF_ROWS.index(row)
    x = make_data("std", (row.B, row.C, row.HW), seed=700 + i)
    p = randn(2, row.C, seed=750 + i)
    ws = host_ws(x, row.groups)
    if row.const:
        L = row.C // row.groups * row.HW
        ws.view(-1, 2)[0] = torch.tensor([L * CONST_A, L * (CONST_A * CONST_A)], dtype=torch.float64)
    return dict(ws=ws, gamma=None if row.null else 1.0 + 0.5 * p[0], beta=None if row.null else p[1])


def coef_refs(row, inp, eps=EPS):
    """fp64 mean and scale [B, C] and the fp32 shift; the constant slab's variance is 0 by construction: scale = gamma / sqrt(eps) there"""
    L = row.C // row.groups * row.HW
    mean, rstd = moments(inp["ws"], L, eps)
    if row.const:
        rstd.view(-1)[0] = 1.0 / math.sqrt(eps)
        mean.view(-1)[0] = CONST_A
    mean, rstd = (_chan(t, row.C, row.groups)[..., 0] for t in (mean, rstd))
    g = torch.ones(row.C, dtype=torch.float64) if inp["gamma"] is None else inp["gamma"].double()
    b = torch.zeros(row.C) if inp["beta"] is None else inp["beta"].float()
    return mean, rstd * g[None], b[None].expand(row.B, row.C)


def coef_ratios(coef, mean, scale, shift):
    """coef [B, 3, C] fp32 -> (|mean_f - mean| / (u |mean|), |scale_f - scale| / (2^-22 |scale|), shift bitwise equal)"""
    return (ratio(coef[:, 0], mean, U * mean.abs()), ratio(coef[:, 1], scale, 2.0 ** -22 * scale.abs()),
            torch.equal(coef[:, 2].contiguous().view(torch.int32), shift.contiguous().view(torch.int32)))


def emulate_coef(row, inp, eps=EPS):
    L = row.C // row.groups * row.HW
    mean, rstd = (_chan(t, row.C, row.groups)[..., 0].float() for t in moments(inp["ws"], L, eps))
    g = torch.ones(row.C) if inp["gamma"] is None else inp["gamma"].float()
    b = torch.zeros(row.C) if inp["beta"] is None else inp["beta"].float()
    return torch.stack([mean, rstd * g[None], b[None].expand(row.B, row.C)], 1)


# ---- norm_head_1x1 ---------------------------------------------------------------------------------------------------------------------
HeadRow = collections.namedtuple("HeadRow", "name K B C HW slope bias")
HEAD_ROWS = tuple(HeadRow("K%d-%dx%dx%d%s" % (K, B, C, HW, "" if slope else "-slope0"), K, B, C, HW, slope, bias)
                  for K in (2, 4, 8)
                  for (B, C, HW, slope, bias) in ((2, 1, 4, 0.01, True), (2, 20, 1028, 0.01, False), (3, 32, 4096, 0.01, True), (2, 20, 1028, 0.0, True))
                  ) + (HeadRow("K8-1x1024x64-lds-max", 8, 1, 1024, 64, 0.01, True),)


def head_inputs(row):
    i = HEAD_ROWS.index(row)
    x = make_data("std", (row.B, row.C, row.HW), seed=800 + i)
    p = randn(2, row.C, seed=850 + i)
    mean, rstd = (t.float() for t in moments(host_ws(x, row.C), row.HW, EPS))           # InstanceNorm: one slab per (sample, channel)
    coef = torch.stack([mean, rstd * (1.0 + 0.5 * p[0])[None], p[1][None].expand(row.B, row.C)], 1).contiguous()
    w = randn(row.K, row.C, seed=900 + i) / math.sqrt(row.C)
    return dict(x=x, coef=coef, w=w, bias=randn(row.K, seed=950 + i) if row.bias else None)


def head_refs(x, coef, w, bias, slope, drop_last=False):
    """slope: the float the call passes -> (ref, bar) [B, K, HW] in fp64"""
    C = x.shape[1]
    s = float(np.float32(slope))
    m, sc, sh = (coef[:, j, :, None].double() for j in range(3))
    xd, wd = x.double(), w.double()
    u = (xd - m) * sc + sh
    t = torch.where(u > 0, u, u * s)
    a = (xd - m).abs() * sc.abs() + sh.abs()
    if drop_last:
        t, wd = t[:, :-1], wd[:, :-1]
    bd = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    ref = torch.einsum("kc,bcp->bkp", wd, t) + bd.view(1, -1, 1)
    A = torch.einsum("kc,bcp->bkp", w.double().abs(), a) + bd.abs().view(1, -1, 1)
    return ref, (C + 4) * U * A


def emulate_head(x, coef, w, bias, slope):
    """the kernel's chain in fp32, channel by channel (a multiply and an add where the kernel fuses them)"""
    B, C, HW = x.shape
    K = w.shape[0]
    s = torch.tensor(slope, dtype=torch.float32)
    acc = (torch.zeros(K) if bias is None else bias.float()).view(1, K, 1).expand(B, K, HW).clone()
    for c in range(C):
        u = (x[:, c] - coef[:, 0, c, None]) * coef[:, 1, c, None] + coef[:, 2, c, None]
        t = torch.where(u > 0, u, u * s)
        acc = acc + w[:, c].view(1, K, 1) * t[:, None, :]
    return acc
