"""The four direct small-channel convolution kernels -- conv_small_cin_kernel, conv3x3_small_cout_kernel, conv3x3_small_cout_norm2_kernel
(csrc/conv_direct.hip) and stem_block_kernel (csrc/conv_stem.hip) -- held to the fmaf chain their source promises, bit for bit, in all 18
instantiations.

entry point -> kernel <template arguments>                                             rows
  cf_conv2d_small_cin, K 3, Cin 1 / 2 / 6      conv_small_cin_kernel<1,3,8> <2,3,4> <6,3,2>       test_small_cin_chain, test_small_cin_statistics
  cf_conv2d_small_cin, K 1, Cin 1 / 2 / 6      conv_small_cin_kernel<1,1,8> <2,1,8> <6,1,8>       the same
  cf_conv2d_small_cout, Cout 1..4              conv3x3_small_cout_kernel<Cout,8>                  test_small_cout_chain
  cf_conv2d_small_cout_norm2, Cout 1..4        conv3x3_small_cout_norm2_kernel<Cout,8>            test_norm2_identity_arm, test_norm2_general_arm
  cf_stem_block / cf_stem_block_y, Cin 1 / 6   stem_block_kernel<1,8,true|false> <6,4,true|false> test_stem_block_chains
The template arguments follow from (Cin, K), from Cout and from (Cin, r given or not) alone: every row names the arguments it passes.

Reference (tests/_fma_chain.py, held to libm's fmaf in test_fma_chain_cpu.py): direct_conv_reference, one chain per output -- the accumulator
starts at the bias, walks ci, then ky, then kx, a tap in the zero padding contributes fma(w, 0, acc), a residual is one more rounded fp32
addition.  Every comparison of outputs is torch.equal on the int32 views; nothing is excluded and nothing has a tolerance.  (Where the
reference holds a NaN -- the +Inf weight rows -- the NaN masks must agree and every other element must agree in its bits: IEEE leaves a NaN's
payload open.)

How the kernels are called: the C entry points of cineflow._lib.lib() on raw pointers into larger buffers.  Every input, weight, bias and
table sits an odd number of floats into a NaN-filled buffer (the kernels promise nothing beyond 4-byte alignment; a read outside an operand
shows as a NaN), every output and every statistics workspace an odd number of elements into a sentinel-filled buffer with at least one block
of the kernel (64 + 4 PY W elements) of sentinel on either side, and after every call the sentinels must be intact and the inputs unchanged.

Shapes, with R = 4 PY rows per block (32, 16 or 8): (1, 1), (2, 65), (R - 1, 63), (R, 64) with one sample, (R + 1, 65) and (2 R + 3, 130)
with three: the smallest maps that put a pixel on every side of every block edge, in rows and in columns (130 = 2 x 64 + 2: three block
columns, the halo column of a block at bx0 = 64 and at 128).  Channels: small_cin to 5 and 6 channels (chain) and to 64 and 128 (statistics:
groups 1, 64 = one channel per group at 64 channels, two at 128); small_cout and norm2 from 1 (no prefetch trip), 2, 5 (odd: the last
channel lands in LDS plane 0) and 64 input channels.

norm2.  Identity arm: tables coef2 = {0, 0, 0}, coefr = {0, 1, 0} and a finite random y2 make the staged value exactly r -- (a - 0) 0 + 0 = +0
contracted or not, gelu_as(+0) = +0, (q - 0) 1 + 0 = q, +0 + q = q for q != 0 -- so the output must equal direct_conv_reference(r, w, bias)
and cf_conv2d_small_cout(r, ...) bit for bit: tile, halo, LDS plane and FMA order of every Cout, shape and Cin parity.  General arm: random
tables, distinct per sample and channel, against GELU_erf((a - m2) s2 + b2) + (q - mr) sr + br and the convolution in fp64 from the same
fp32 tables, at the bar tests/test_gpu_flow_head.py holds this kernel to: 2e-5 absolute at outputs of unit scale.

Statistics (small_cin, both stem forms): fp64 sums of the kernel's OWN output at the existing bar, 2e-6 of (the group's absolute sum + 1)
(test_gpu_stem_block.py, test_gpu_ops.py).  A positive gn_groups is asked on a workspace pre-filled with garbage of magnitude 1e6 (the
memset is what passes), the stem's negative gn_groups twice on a zeroed one (it must add).  On maps of one block (H <= R, W <= 64) the stem's
statistics are the same bits in two runs and in both forms, as conv_stem.hip promises; conv_small_cin_kernel sums through LDS fp32 atomics and
promises no such thing.

One row leaves that list of maps, in its sample count alone: test_norm2_planes_with_every_compute_unit_full runs 2048 samples of 32 x 64.  The
two LDS planes of the norm2 kernel guard against a race between waves of one workgroup, and waves drift apart only where several
workgroups share a SIMD; on the maps above (27 workgroups at the most, on 256 compute units) a kernel with ONE plane passes every row.

Mutations (scratch builds, every access inside its buffer; "old" = test_gpu_stem_block.py, test_gpu_flow_head.py, test_gpu_stem_apply.py and
the small_cin / small_cout tests of test_gpu_ops.py, 57 tests, on the same library):
  1. ky and kx loops of conv_small_cin_kernel swapped     142 rows here fail (every 3x3 small_cin and stem row but the one-pixel maps); old: 14 fail
                                                          (the stem against the mutated small_cin); test_gpu_ops.py's small_cin tests pass
  2. small_cout's fmaf as acc += wv * in, no contraction  183 fail (small_cout rows, the centre-tap row, norm2 against small_cout); old: all 57 pass
  3. norm2 reads its halo columns mirrored                162 fail (both arms); old: 5 fail
  4. norm2 stages every channel into plane 0              the full-occupancy row fails (611 and 1536 elements); every other row and old pass
  5. the stem's 1x1 chain from 0, bias added last         59 of 60 stem rows fail; old: 22 fail (the stem's r against small_cin's, bit for bit)

Measured on the MI355X: profiles/direct_conv_table.md (pytest -s prints one line per row).
The argument checks of these entry points run without a device: tests/test_abi_and_host.py::test_direct_conv_argument_checks_need_no_gpu.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _fma_chain import DOUBLE_ROUNDING_TRIPLES, direct_conv_reference, fma32, fma32_plain

pytestmark = pytest.mark.gpu

SENT = -12345.5
NAN = float("nan")
INF = float("inf")
STATS_BAR = 2e-6                                       # of (the group's absolute sum + 1): test_gpu_stem_block.py, test_gpu_ops.py
NORM2_BAR = 2e-5                                       # absolute, outputs of unit scale: test_gpu_flow_head.py
I32 = torch.int32


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def randn_nonzero(*shape, seed):
    t = randn(*shape, seed=seed)
    t[t == 0] = 0.5
    return t


def shapes(PY):
    """(B, H, W) around every edge of a 64 x (4 PY) block"""
    R = 4 * PY
    return [(1, 1, 1), (1, 2, 65), (1, R - 1, 63), (1, R, 64), (3, R + 1, 65), (3, 2 * R + 3, 130)]


NSHAPES = 6


def single_block(PY, H, W):
    return H <= 4 * PY and W <= 64


def bits_differ(got, want):
    return int((got.contiguous().view(I32) != want.contiguous().view(I32)).sum())


def assert_bits(got, want, what):
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, what
    bad = bits_differ(got, want)
    assert bad == 0 and torch.equal(got.contiguous().view(I32), want.contiguous().view(I32)), "%s: %d of %d elements differ in their bits" % (what, bad, got.numel())


def assert_bits_or_nan(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN at %d elements, the chain has %d" % (what, int(torch.isnan(got).sum()), int(nan.sum()))
    assert_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), what)


class Fences:
    """device operands of one call, each an odd number of elements into a buffer of its own: inputs fenced by NaN, outputs by SENT"""

    def __init__(self, dev, PY, W):
        self.dev, self.pad, self.held = dev, (64 + 4 * PY * W) | 1, []

    def _view(self, shape, dtype, fence):
        n = int(np.prod(shape))
        buf = torch.full((2 * self.pad + n,), fence, dtype=dtype, device=self.dev)
        v = buf[self.pad:self.pad + n].view(shape)
        assert v.is_contiguous() and v.data_ptr() % (2 * v.element_size()) == v.element_size()
        return buf, v, n

    def put(self, t):
        """an input (None stays None)"""
        if t is None:
            return None
        buf, v, n = self._view(t.shape, t.dtype, NAN)
        v.copy_(t)
        self.held.append((buf, n, NAN, t.clone()))
        return v

    def new(self, shape, dtype=torch.float32, fill=NAN):
        """an output, pre-filled with `fill` (a number or a tensor)"""
        buf, v, n = self._view(shape, dtype, SENT)
        v.copy_(fill) if isinstance(fill, torch.Tensor) else v.fill_(fill)
        self.held.append((buf, n, SENT, None))
        return v

    def check(self):
        for buf, n, fence, data in self.held:
            host = buf.cpu()
            edge = torch.cat([host[:self.pad], host[self.pad + n:]])
            assert bool(torch.isnan(edge).all() if fence != fence else (edge == fence).all()), "the kernel wrote outside an operand of %d elements" % n
            if data is not None:
                inner = host[self.pad:self.pad + n].view(data.shape)
                assert bool(((inner == data) | (torch.isnan(inner) & torch.isnan(data))).all()), "an input changed"


def ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    from cineflow._lib import lib
    h = lib()
    rc = getattr(h, name)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc, h.cf_last_error())
    torch.cuda.synchronize()


def garbage(*shape):
    return (randn(*shape, seed=4242) * 1e6).double()


def run_small_cin(dev, x, w, bias, PY, groups=0, ws_fill=None, ws_null=False):
    """cf_conv2d_small_cin -> (out, ws [B, groups, 2] or None) on the CPU; ws_fill None: garbage"""
    B, Cin, H, W = x.shape
    Cout, K = w.shape[0], w.shape[2]
    f = Fences(dev, PY, W)
    xd, wd, bd = f.put(x), f.put(w), f.put(bias)
    out = f.new((B, Cout, H, W))
    ws = None
    if groups and not ws_null:
        ws = f.new((B, groups, 2), torch.float64, garbage(B, groups, 2) if ws_fill is None else ws_fill)
    call("cf_conv2d_small_cin", ptr(xd), ptr(wd), ptr(bd), ptr(out), B, Cin, H, W, Cout, K, ptr(ws), groups)
    f.check()
    return out.cpu(), None if ws is None else ws.cpu()


def run_small_cout(dev, x, w, bias, res):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    f = Fences(dev, 8, W)
    xd, wd, bd, rd = f.put(x), f.put(w), f.put(bias), f.put(res)
    out = f.new((B, Cout, H, W))
    call("cf_conv2d_small_cout", ptr(xd), ptr(wd), ptr(bd), ptr(rd), ptr(out), B, Cin, H, W, Cout)
    f.check()
    return out.cpu()


def run_norm2(dev, y2, c2, r, cr, w, bias):
    B, Cin, H, W = r.shape
    Cout = w.shape[0]
    assert tuple(c2.shape) == tuple(cr.shape) == (B, 3, Cin) and y2.shape == r.shape
    f = Fences(dev, 8, W)
    yd, c2d, rd, crd, wd, bd = f.put(y2), f.put(c2), f.put(r), f.put(cr), f.put(w), f.put(bias)
    out = f.new((B, Cout, H, W))
    call("cf_conv2d_small_cout_norm2", ptr(yd), ptr(c2d), ptr(rd), ptr(crd), ptr(wd), ptr(bd), ptr(out), B, Cin, H, W, Cout)
    f.check()
    return out.cpu()


def identity_tables(B, Cin):
    """coef2 = {m 0, s 0, b 0}, coefr = {m 0, s 1, b 0}: the staged value is r"""
    c2 = torch.zeros(B, 3, Cin)
    cr = torch.zeros(B, 3, Cin)
    cr[:, 1] = 1.0
    return c2, cr


def run_norm2_identity(dev, r, w, bias, seed=77):
    """cf_conv2d_small_cout_norm2 on the identity tables and a finite random y2: a convolution of r"""
    c2, cr = identity_tables(*r.shape[:2])
    return run_norm2(dev, randn(*r.shape, seed=seed) * 1.5 + 0.3, c2, r, cr, w, bias)


def run_stem(dev, x, w3, b3, w1, b1, groups, store_r=True, zeroed_calls=0):
    """cf_stem_block (store_r) or cf_stem_block_y -> (y, r or None, ws_y, ws_r) on the CPU.  zeroed_calls = 0: one call with a positive gn_groups
    on workspaces full of garbage; n > 0: n calls with -gn_groups on workspaces zeroed here"""
    B, Cin, H, W = x.shape
    Cout = w3.shape[0]
    PY = 8 if Cin == 1 else 4
    f = Fences(dev, PY, W)
    xd, w3d, b3d, w1d, b1d = f.put(x), f.put(w3), f.put(b3), f.put(w1), f.put(b1)
    y = f.new((B, Cout, H, W))
    r = f.new((B, Cout, H, W)) if store_r else None
    fill = 0.0 if zeroed_calls else garbage(B, groups, 2)
    ws_y, ws_r = f.new((B, groups, 2), torch.float64, fill), f.new((B, groups, 2), torch.float64, fill)
    for _ in range(max(1, zeroed_calls)):
        g = -groups if zeroed_calls else groups
        if store_r:
            call("cf_stem_block", ptr(xd), ptr(w3d), ptr(b3d), ptr(w1d), ptr(b1d), ptr(y), ptr(r), B, Cin, H, W, Cout, ptr(ws_y), ptr(ws_r), g)
        else:
            call("cf_stem_block_y", ptr(xd), ptr(w3d), ptr(b3d), ptr(w1d), ptr(b1d), ptr(y), B, Cin, H, W, Cout, ptr(ws_y), ptr(ws_r), g)
    f.check()
    return y.cpu(), None if r is None else r.cpu(), ws_y.cpu(), ws_r.cpu()


def stats_of(out, groups):
    """({sum, sum of squares} [B, groups, 2], the bar's scale [B, groups, 1]) of a kernel's own output, in fp64"""
    B = out.shape[0]
    d = out.double().reshape(B, groups, -1)
    return torch.stack([d.sum(-1), (d * d).sum(-1)], -1), d.abs().sum(-1)[..., None] + 1.0


def stats_ratio(ws, out, groups, times=1):
    """worst |ws - times x fp64 sums| / (STATS_BAR x times x (the group's absolute sum + 1))"""
    want, scale = stats_of(out, groups)
    return float(((ws - times * want).abs() / (STATS_BAR * times * scale)).max())


def some_channels(cout):
    """the channels of a wide output that are walked on the CPU: both ends, and both sides of the middle"""
    return list(range(cout)) if cout <= 6 else [0, 1, cout // 2 - 1, cout // 2, cout - 1]


# ================================================================================================================== small_cin
SMALL_CIN = [(1, 3, 8), (2, 3, 4), (6, 3, 2), (1, 1, 8), (2, 1, 8), (6, 1, 8)]          # CIN, KS, PY of launch_small_cin
_CIN_CASES = {}


def small_cin_case(cin, K, PY, si, cout):
    """operands and the chain (of some_channels) with and without the bias, made once and left unchanged"""
    key = (cin, K, PY, si, cout)
    if key not in _CIN_CASES:
        B, H, W = shapes(PY)[si]
        seed = 7000 + 100 * SMALL_CIN.index((cin, K, PY)) + 10 * si + (cout % 7)
        x, w, b = randn(B, cin, H, W, seed=seed), randn(cout, cin, K, K, seed=seed + 1) / math.sqrt(cin * K * K), randn(cout, seed=seed + 2)
        ch = some_channels(cout)
        _CIN_CASES[key] = dict(x=x, w=w, b=b, ch=ch, with_b=direct_conv_reference(x, w[ch], b[ch])[0], without=direct_conv_reference(x, w[ch], None)[0])
    return _CIN_CASES[key]


@pytest.mark.parametrize("cout", [5, 6])
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cin,K,PY", SMALL_CIN)
def test_small_cin_chain(dev, cin, K, PY, si, cout):
    c = small_cin_case(cin, K, PY, si, cout)
    B, H, W = shapes(PY)[si]
    got_b, _ = run_small_cin(dev, c["x"], c["w"], c["b"], PY)
    got_0, _ = run_small_cin(dev, c["x"], c["w"], None, PY)
    print("\nsmall_cin<%d,%d,%d> %d x %d x %d x %d -> %d: %d (bias) and %d (no bias) of %d elements differ from the chain" % (
        cin, K, PY, B, cin, H, W, cout, bits_differ(got_b, c["with_b"]), bits_differ(got_0, c["without"]), got_b.numel()))
    assert_bits(got_b, c["with_b"], "bias")
    assert_bits(got_0, c["without"], "no bias")


@pytest.mark.parametrize("cout,groups", [(64, 1), (64, 64), (128, 1), (128, 64)])
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cin,K,PY", SMALL_CIN)
def test_small_cin_statistics(dev, cin, K, PY, si, cout, groups):
    """the output with statistics is the output without (every channel), which is the chain (some_channels); the workspace, asked on
    garbage and on zeros, holds the fp64 sums of that output inside the bar, and nothing else is written"""
    c = small_cin_case(cin, K, PY, si, cout)
    B, H, W = shapes(PY)[si]
    plain, _ = run_small_cin(dev, c["x"], c["w"], c["b"], PY)
    assert_bits(plain[:, c["ch"]], c["with_b"], "no statistics")
    worst = 0.0
    for fill in (None, 0.0):
        out, ws = run_small_cin(dev, c["x"], c["w"], c["b"], PY, groups, fill)
        assert_bits(out, plain, "statistics asked")
        assert bool(torch.isfinite(ws).all())
        worst = max(worst, stats_ratio(ws, out, groups))
    print("\nsmall_cin<%d,%d,%d> %d x %d x %d x %d -> %d, %d groups: statistics at %.4f of the bar" % (cin, K, PY, B, cin, H, W, cout, groups, worst))
    assert worst <= 1.0


def test_small_cin_without_a_workspace_computes_no_statistics(dev):
    """include/cineflow.h: gn_ws may be NULL, and gn_groups then means nothing, whatever it holds"""
    c = small_cin_case(2, 3, 4, 4, 6)
    for groups in (3, 65, -1):
        out, ws = run_small_cin(dev, c["x"], c["w"], c["b"], 4, groups, ws_null=True)
        assert ws is None
        assert_bits(out, c["with_b"], "gn_ws NULL, gn_groups %d" % groups)


# ================================================================================================================== small_cout, norm2
HEAD_CIN = [1, 2, 5, 64]
_HEAD_CASES = {}


def head_case(cin, si):
    """operands for four output channels (a call to Cout = c takes the first c) and the chains, made once and left unchanged; x has no zero"""
    key = (cin, si)
    if key not in _HEAD_CASES:
        B, H, W = shapes(8)[si]
        seed = 8000 + 100 * HEAD_CIN.index(cin) + 10 * si
        x, w, b = randn_nonzero(B, cin, H, W, seed=seed), randn(4, cin, 3, 3, seed=seed + 1) / math.sqrt(9 * cin), randn(4, seed=seed + 2)
        res = randn(B, 4, H, W, seed=seed + 3)
        with_b = direct_conv_reference(x, w, b)[0]
        with_b_res = with_b + res                      # direct_conv_reference(x, w, b, res): one fp32 addition; the chain is not walked a third time
        assert with_b_res.dtype == torch.float32
        if cin < 64:
            assert torch.equal(with_b_res, direct_conv_reference(x, w, b, res)[0])
        _HEAD_CASES[key] = dict(x=x, w=w, b=b, res=res, with_b=with_b, with_b_res=with_b_res, without=direct_conv_reference(x, w, None)[0])
    return _HEAD_CASES[key]


@pytest.mark.parametrize("cin", HEAD_CIN)
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_small_cout_chain(dev, cout, si, cin):
    c = head_case(cin, si)
    B, H, W = shapes(8)[si]
    w, b, res = c["w"][:cout].contiguous(), c["b"][:cout].contiguous(), c["res"][:, :cout].contiguous()
    rows = [("bias, res", b, res, c["with_b_res"]), ("bias", b, None, c["with_b"]), ("plain", None, None, c["without"])]
    got = [run_small_cout(dev, c["x"], w, bb, rr) for _, bb, rr, _ in rows]
    print("\nsmall_cout<%d,8> %d x %d x %d x %d: %s of %d elements differ from the chain" % (
        cout, B, cin, H, W, ", ".join("%d (%s)" % (bits_differ(g, want[:, :cout]), name) for g, (name, _, _, want) in zip(got, rows)), got[0].numel()))
    for g, (name, _, _, want) in zip(got, rows):
        assert_bits(g, want[:, :cout].contiguous(), name)


@pytest.mark.parametrize("cin", HEAD_CIN)
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_norm2_identity_arm(dev, cout, si, cin):
    c = head_case(cin, si)
    B, H, W = shapes(8)[si]
    assert bool((c["x"] != 0).all())
    w, b = c["w"][:cout].contiguous(), c["b"][:cout].contiguous()
    got_b, got_0 = run_norm2_identity(dev, c["x"], w, b), run_norm2_identity(dev, c["x"], w, None, seed=78)
    print("\nnorm2<%d,8> identity arm %d x %d x %d x %d: %d (bias) and %d (no bias) of %d elements differ from the chain" % (
        cout, B, cin, H, W, bits_differ(got_b, c["with_b"][:, :cout]), bits_differ(got_0, c["without"][:, :cout]), got_b.numel()))
    assert_bits(got_b, c["with_b"][:, :cout].contiguous(), "bias")
    assert_bits(got_0, c["without"][:, :cout].contiguous(), "no bias")
    assert_bits(got_b, run_small_cout(dev, c["x"], w, b, None), "against cf_conv2d_small_cout")


@pytest.mark.parametrize("cout", [1, 4])
def test_norm2_planes_with_every_compute_unit_full(dev, cout):
    """2048 samples of one block each (32 x 64, 8 channels): several workgroups share every SIMD, so the waves of a workgroup drift apart
    between two barriers -- the setting in which the second LDS plane is what keeps a fast wave's next channel out of a slow wave's reads.
    The maps above leave most compute units idle and their waves in step.  Identity arm against cf_conv2d_small_cout (held to the chain
    above), on the device; the operands are made there."""
    B, Cin, H, W = 2048, 8, 32, 64
    g = torch.Generator(device=dev).manual_seed(12000 + cout)
    r = torch.randn(B, Cin, H, W, device=dev, generator=g)
    r[r == 0] = 0.5
    y2 = torch.randn(B, Cin, H, W, device=dev, generator=g)
    w, b = (randn(cout, Cin, 3, 3, seed=12001) / math.sqrt(9 * Cin)).to(dev), randn(cout, seed=12002).to(dev)
    c2, cr = (t.to(dev) for t in identity_tables(B, Cin))
    f = Fences(dev, 8, W)
    out, want = f.new((B, cout, H, W)), f.new((B, cout, H, W))
    call("cf_conv2d_small_cout", ptr(r), ptr(w), ptr(b), None, ptr(want), B, Cin, H, W, cout)
    call("cf_conv2d_small_cout_norm2", ptr(y2), ptr(c2), ptr(r), ptr(cr), ptr(w), ptr(b), ptr(out), B, Cin, H, W, cout)
    f.check()
    bad = int((out.view(I32) != want.view(I32)).sum())
    print("\nnorm2<%d,8> identity arm, %d blocks of 8 channels: %d of %d elements differ from cf_conv2d_small_cout" % (cout, B, bad, out.numel()))
    assert bad == 0 and not bool(torch.isnan(out).any())


_GENERAL = {}


def general_case(cin, si):
    """random tables, distinct per sample and channel, and the fp64 evaluation from the same fp32 values"""
    key = (cin, si)
    if key not in _GENERAL:
        B, H, W = shapes(8)[si]
        seed = 9000 + 100 * HEAD_CIN.index(cin) + 10 * si
        y2, r = randn(B, cin, H, W, seed=seed) * 1.5 + 0.3, randn(B, cin, H, W, seed=seed + 1) * 0.7 - 0.2
        c2 = torch.stack([0.3 * randn(B, cin, seed=seed + 2), 1.0 + 0.3 * randn(B, cin, seed=seed + 3), 0.2 * randn(B, cin, seed=seed + 4)], 1).contiguous()
        cr = torch.stack([0.3 * randn(B, cin, seed=seed + 5), 1.0 + 0.3 * randn(B, cin, seed=seed + 6), 0.2 * randn(B, cin, seed=seed + 7)], 1).contiguous()
        w, b = randn(4, cin, 3, 3, seed=seed + 8) / math.sqrt(9 * cin), randn(4, seed=seed + 9)
        t2, tr = c2.double()[..., None, None], cr.double()[..., None, None]
        u = (y2.double() - t2[:, 0]) * t2[:, 1] + t2[:, 2]
        v = 0.5 * u * (1.0 + torch.special.erf(u / math.sqrt(2.0))) + (r.double() - tr[:, 0]) * tr[:, 1] + tr[:, 2]
        _GENERAL[key] = dict(y2=y2, r=r, c2=c2, cr=cr, w=w, b=b, want=F.conv2d(v, w.double(), b.double(), padding=1))
    return _GENERAL[key]


@pytest.mark.parametrize("cin", HEAD_CIN)
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_norm2_general_arm(dev, cout, si, cin):
    c = general_case(cin, si)
    B, H, W = shapes(8)[si]
    got = run_norm2(dev, c["y2"], c["c2"], c["r"], c["cr"], c["w"][:cout].contiguous(), c["b"][:cout].contiguous())
    want = c["want"][:, :cout]
    d = float((got.double() - want).abs().max())
    print("\nnorm2<%d,8> general arm %d x %d x %d x %d: max|out - fp64| = %.3e (bar %.0e; outputs up to %.2f)" % (cout, B, cin, H, W, d, NORM2_BAR, float(want.abs().max())))
    # unit scale, as the data the bar was set on: 9 Cin taps of variance 1 / (9 Cin) on values of rms about 1.6.  (A guard on the operands:
    # with a few taps the extremes run to several times the rms, so the rms is what is held.)
    assert float((want * want).mean().sqrt()) < 4.0
    assert d <= NORM2_BAR


# ================================================================================================================== stem
STEM = [(1, 8), (6, 4)]                                # CIN, PY of launch_stem_block; STORE_R true and false in every row
_STEM_CASES = {}


def stem_case(cin, si, cout):
    key = (cin, si, cout)
    if key not in _STEM_CASES:
        B, H, W = shapes(dict(STEM)[cin])[si]
        seed = 10000 + 1000 * cin + 10 * si + (cout % 7)
        x = randn(B, cin, H, W, seed=seed)
        w3, w1 = randn(cout, cin, 3, 3, seed=seed + 1) / math.sqrt(9 * cin), randn(cout, cin, 1, 1, seed=seed + 2) / math.sqrt(cin)
        b3, b1 = randn(cout, seed=seed + 3), randn(cout, seed=seed + 4)
        ch = some_channels(cout)
        _STEM_CASES[key] = dict(x=x, w3=w3, b3=b3, w1=w1, b1=b1, ch=ch, y=direct_conv_reference(x, w3[ch], b3[ch])[0], r=direct_conv_reference(x, w1[ch], b1[ch])[0],
                                y0=direct_conv_reference(x, w3[ch], None)[0], r0=direct_conv_reference(x, w1[ch], None)[0])
    return _STEM_CASES[key]


@pytest.mark.parametrize("cout,groups", [(5, 1), (6, 6), (64, 1), (64, 64), (128, 64)])
@pytest.mark.parametrize("si", range(NSHAPES))
@pytest.mark.parametrize("cin,PY", STEM)
def test_stem_block_chains(dev, cin, PY, si, cout, groups):
    c = stem_case(cin, si, cout)
    B, H, W = shapes(PY)[si]
    x, w3, b3, w1, b1, ch = (c[k] for k in ("x", "w3", "b3", "w1", "b1", "ch"))
    y, r, ws_y, ws_r = run_stem(dev, x, w3, b3, w1, b1, groups)
    print("\nstem<%d,%d,true|false> %d x %d x %d x %d -> 2 x %d, %d groups: %d (y) and %d (r) of %d elements differ from the chain" % (
        cin, PY, B, cin, H, W, cout, groups, bits_differ(y[:, ch], c["y"]), bits_differ(r[:, ch], c["r"]), c["y"].numel()))
    assert_bits(y[:, ch], c["y"], "y")
    assert_bits(r[:, ch], c["r"], "r")
    # every channel: cf_conv2d_small_cin's maps (anchored in test_small_cin_chain), and the form that does not store r
    assert_bits(y, run_small_cin(dev, x, w3, b3, PY)[0], "y against cf_conv2d_small_cin")
    assert_bits(r, run_small_cin(dev, x, w1, b1, 8)[0], "r against cf_conv2d_small_cin")
    y_only, none, ws_y2, ws_r2 = run_stem(dev, x, w3, b3, w1, b1, groups, store_r=False)
    assert none is None
    assert_bits(y_only, y, "cf_stem_block_y's y")
    # no bias
    y0, r0, _, _ = run_stem(dev, x, w3, None, w1, None, groups)
    assert_bits(y0[:, ch], c["y0"], "y, no bias")
    assert_bits(r0[:, ch], c["r0"], "r, no bias")
    # statistics: garbage workspaces and a positive gn_groups (both forms); zeroed ones and a negative gn_groups, twice: it adds
    _, _, ws_yn, ws_rn = run_stem(dev, x, w3, b3, w1, b1, groups, zeroed_calls=1)
    _, _, ws_yt, ws_rt = run_stem(dev, x, w3, b3, w1, b1, groups, store_r=False, zeroed_calls=2)
    ratios = [stats_ratio(ws, out, groups) for ws, out in ((ws_y, y), (ws_r, r), (ws_y2, y), (ws_r2, r), (ws_yn, y), (ws_rn, r))]
    ratios += [stats_ratio(ws_yt, y, groups, times=2), stats_ratio(ws_rt, r, groups, times=2)]
    print("stem<%d,%d> %d groups: statistics at %.4f of the bar" % (cin, PY, groups, max(ratios)))
    assert all(bool(torch.isfinite(w).all()) for w in (ws_y, ws_r, ws_y2, ws_r2, ws_yn, ws_rn, ws_yt, ws_rt))
    assert max(ratios) <= 1.0, ratios
    if single_block(PY, H, W):
        # one block per sample: its contribution is the same bits in every run and in both forms, and one fp64 addition to 0 keeps them
        again = run_stem(dev, x, w3, b3, w1, b1, groups)
        for name, a, b in (("ws_y, second run", again[2], ws_y), ("ws_r, second run", again[3], ws_r), ("ws_y, cf_stem_block_y", ws_y2, ws_y),
                           ("ws_r, cf_stem_block_y", ws_r2, ws_r), ("ws_y, negative gn_groups", ws_yn, ws_y), ("ws_r, negative gn_groups", ws_rn, ws_r),
                           ("ws_y, added twice", ws_yt, 2 * ws_y), ("ws_r, added twice", ws_rt, 2 * ws_r)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name


# ================================================================================================================== arithmetic edges
def test_fmaf_not_mul_add_small_cin(dev):
    """Cin 1, K 1, Cout 12: out[m, p] = fma(w[m], x[p], bias[m]).  The image holds every a of DOUBLE_ROUNDING_TRIPLES, channel m carries (b, c)
    of row m: at (m, the pixel of a_m) the fmaf value and the twice-rounded one differ"""
    a, b, c = (torch.from_numpy(v.copy()) for v in DOUBLE_ROUNDING_TRIPLES.T)
    x, w = a.view(1, 1, 3, 4), b.view(12, 1, 1, 1)
    got, _ = run_small_cin(dev, x, w, c, 8)
    assert_bits(got, direct_conv_reference(x, w, c)[0], "chain")
    diag = got.view(12, 12).diagonal()
    want, plain = (torch.from_numpy(f(*DOUBLE_ROUNDING_TRIPLES.T)) for f in (fma32, fma32_plain))
    assert bits_differ(want, plain) == 12
    assert_bits(diag.contiguous(), want, "fmaf")
    assert bits_differ(diag.contiguous(), plain) == 12


@pytest.mark.parametrize("family", ["small_cout", "norm2"])
def test_fmaf_not_mul_add_centre_tap(dev, family):
    """the same rows as the centre tap of a 3x3 head, every other weight 0, four rows a launch: bias c, fma(0, x, c) = c up to the centre,
    fma(b, a, c) there, unchanged after"""
    a, b, c = (torch.from_numpy(v.copy()) for v in DOUBLE_ROUNDING_TRIPLES.T)
    x = a.view(1, 1, 3, 4)
    want, plain = (torch.from_numpy(f(*DOUBLE_ROUNDING_TRIPLES.T)) for f in (fma32, fma32_plain))
    for j in range(3):
        rows = slice(4 * j, 4 * j + 4)
        w = torch.zeros(4, 1, 3, 3)
        w[:, 0, 1, 1] = b[rows]
        bias = c[rows].contiguous()
        got = run_small_cout(dev, x, w, bias, None) if family == "small_cout" else run_norm2_identity(dev, x, w, bias)
        assert_bits(got, direct_conv_reference(x, w, bias)[0], "chain")
        diag = got.view(4, 12)[:, rows].diagonal().contiguous()
        assert_bits(diag, want[rows].contiguous(), "fmaf")
        assert bits_differ(diag, plain[rows].contiguous()) == 4


FAMILIES = ["small_cin_3x3", "small_cin_1x1", "small_cout", "norm2", "stem"]


def run_family(dev, family, x, w, bias):
    """one launch of `family` on (x, w, bias) -> output; the stem gets w as its 3x3 weights and w's centre taps as its 1x1 weights and returns y"""
    if family.startswith("small_cin"):
        return run_small_cin(dev, x, w, bias, {(1, 3): 8, (2, 3): 4, (6, 3): 2}.get((x.shape[1], w.shape[2]), 8))[0]
    if family == "small_cout":
        return run_small_cout(dev, x, w, bias, None)
    if family == "norm2":
        return run_norm2_identity(dev, x, w, bias)
    return run_stem(dev, x, w, bias, w[:, :, 1:2, 1:2].contiguous(), bias, 1)[0]


def family_operands(family, B, H, W, seed):
    cin, cout, K = {"small_cin_3x3": (2, 5, 3), "small_cin_1x1": (6, 5, 1), "small_cout": (5, 3, 3), "norm2": (5, 3, 3), "stem": (6, 5, 3)}[family]
    return randn_nonzero(B, cin, H, W, seed=seed), randn_nonzero(cout, cin, K, K, seed=seed + 1) / math.sqrt(cin * K * K), randn(cout, seed=seed + 2)


@pytest.mark.parametrize("family", FAMILIES)
def test_subnormals_are_kept(dev, family):
    """x 1e-25, w 1e-15, bias 1e-40: every product, partial sum and output lies below 2^-126.  Gradual underflow: the chain keeps them, a
    kernel that flushes its operands or results differs on every element"""
    x, w, b = family_operands(family, 1, 9, 70, 11000)
    x, w, b = x * 1e-25, w * math.sqrt(w[0].numel()) * 1e-15, b * 1e-40
    assert 0 < float(b.abs().max()) < 2.0 ** -126
    for bias in (b, None):
        want = direct_conv_reference(x, w, bias)[0]
        assert bool((want.abs() < 2.0 ** -126).all()) and float((want != 0).float().mean()) > 0.99, "the row is meant to give subnormal outputs"
        got = run_family(dev, family, x, w, bias)
        assert_bits(got, want, "%s, subnormal outputs" % family)
    if family == "stem":
        w1 = w[:, :, 1:2, 1:2].contiguous()
        assert_bits(run_stem(dev, x, w, b, w1, b, 1)[1], direct_conv_reference(x, w1, b)[0], "stem r, subnormal outputs")


@pytest.mark.parametrize("family", ["small_cin_3x3", "small_cout", "norm2", "stem"])
def test_inf_weight_meets_the_padding(dev, family):
    """positive x, every weight of output channel 0 +Inf, 33 x 65 (two block rows, two block columns): an interior output of channel 0 is
    +Inf, one whose window touches the padding is NaN -- fma(Inf, 0, acc) -- and the zero of each kernel's padding is a real zero: the
    compared 0 of small_cin and the stem, the buffer range check of small_cout, the zeroed LDS of norm2.  The other channels stay finite."""
    x, w, b = family_operands(family, 1, 33, 65, 11100)
    x = x.abs() + 0.1
    w[0] = INF
    want = direct_conv_reference(x, w, b)[0]
    edge = torch.ones(33, 65, dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    assert torch.equal(torch.isnan(want[0, 0]), edge) and bool((want[0, 0][~edge] == INF).all()) and bool(torch.isfinite(want[0, 1:]).all())
    got = run_family(dev, family, x, w, b)
    assert_bits_or_nan(got, want, family)


@pytest.mark.parametrize("family", ["small_cin_3x3", "small_cin_1x1", "small_cout", "norm2", "stem"])
def test_nan_stays_in_its_sample(dev, family):
    """3 samples of 33 x 65, a NaN in sample 1: samples 0 and 2 are the clean run's bits, their statistics rows finite and inside the bar"""
    x, w, b = family_operands(family, 3, 33, 65, 11200)
    xn = x.clone()
    xn[1, -1, 7, 9] = NAN
    groups = 1
    if family.startswith("small_cin"):
        PY = 4 if family == "small_cin_3x3" else 8
        runs = [run_small_cin(dev, t, w, b, PY, groups) for t in (x, xn)]
        outs, wss = [[r[0]] for r in runs], [[r[1]] for r in runs]
    elif family == "stem":
        runs = [run_stem(dev, t, w, b, w[:, :, 1:2, 1:2].contiguous(), b, groups) for t in (x, xn)]
        outs, wss = [[r[0], r[1]] for r in runs], [[r[2], r[3]] for r in runs]
    else:
        outs, wss = [[run_family(dev, family, t, w, b)] for t in (x, xn)], [[], []]
    for clean, dirty in zip(*outs):
        assert_bits(dirty[0::2].contiguous(), clean[0::2].contiguous(), "%s: samples 0 and 2" % family)
        assert bool(torch.isnan(dirty[1]).any()) and not bool(torch.isnan(clean).any())
    for out, ws in zip(outs[1], wss[1]):
        assert bool(torch.isfinite(ws[0::2]).all()) and bool(torch.isnan(ws[1]).all())
        assert stats_ratio(ws[0::2], out[0::2], groups) <= 1.0
