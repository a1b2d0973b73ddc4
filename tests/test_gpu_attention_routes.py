"""cf_attention_cf / cf_attention_cf_masked on all seven kernels they can launch, each row held to the fp64 reference of its own arithmetic
and to the route probe.

entry point -> kernel -> rows (the table itself is _attention_refs.ROWS, shared with the CPU tests of the reference)
  cf_attention_cf_route == 1   attention_cf_f16s_kernel<16|32|64>   d >= 16 and every 8-key group of V 16-byte aligned
  cf_attention_cf_route == 0   attention_cf_kernel<8|16|32|64>      d == 8; d >= 16 through a V that is 4 bytes off
The launcher dispatches on cf_attention_cf_route itself; every row asks the probe first and fails if it names another kernel than the row
does, so a changed alignment rule cannot turn "the f16-split kernel at d = 32" into the fp32 kernel passing in its place.

Every row (C ABI rows).  The output is NaN-filled and lies 64 floats inside a buffer of sentinels that must be untouched on both sides; q and
k sit one float into NaN-fenced buffers and V sits in one too (16-byte aligned on route 1, 4 bytes off on route 0), so a read outside any
of them poisons the result; |out - y| <= bar with y and bar of _attention_refs.attention_refs (derivation in that module's docstring:
bar = (2 e_s + SPLIT_BAR) A_o); and on unit-amplitude rows the suite's standing 2e-5 against fp64 attention of the true operands.  That the
bar resolves what each row is about -- one lo half, one channel, one key on either side of the mask, b and h exchanged, a missing rescale,
another clamp -- is asserted on the CPU, row by row (test_attention_refs_cpu.py); B = 2 and heads = 3 wherever b / h matter.

Rows (B, heads, Nq, Nk):
  blocks   (2, 3, 160, 96), all seven kernels     two query blocks, the second with one active wave of four (the qb / bh split of blockIdx.x);
                                                  three key blocks: both LDS buffers of the f16-split kernel are reused
  mask     (2, 3, 32, 64), nk_valid 33 .. 64      every boundary class of the masked key index (r & 3) + 8 (r >> 2) + 4 half, on f16s d = 16,
           (2, 3, 32, 32), nk_valid 1             64 and fp32 d = 8, 32 (misaligned V).  Each case runs with zero padding and with finite
                                                  garbage in the padded keys (K random x 3, V = 1000): bit-identical outputs, because a masked
                                                  score is -inf, p exactly 0, and 0 x finite adds exactly 0.  One key: the output is its V row
  strides  (2, 3, 64, 64), fp32 d = 8, f16s d = 32   q, k as the halves of one [B, 2C, N] buffer with a separate V (the same_qk call of
                                                  nn.MultiheadAttention), and q, k, v as thirds of [B, 3C, N]: bit-equal to the contiguous
                                                  call.  (The [B, 3C, N] buffer of the f16s row is 16-byte aligned in its fence: V is its third.)
  rescale  (2, 3, 32, 128), f16s d = 64, fp32 d = 8  block maxima ascending for every query (alpha < 1 at every block), descending (alpha == 1
                                                  after the first), and unit normals with q x 8 (one key dominates, the maximum moves often)
  long     (1, 2, 32, 512), f16s d = 64, fp32 d = 8  sixteen key blocks
  clamp    (2, 3, 32, 64), f16s d = 32            |k|, |v| of 65520 .. 1e6: clamped to +-60000 by split_h8, finite output under the bar
  wrapper  ops.attention_cf, (Nq, Nk) in (45, 70) (33, 97) (64, 40) (1, 1), d = 8, 16   the two masked kernels the ragged case of
                                                  test_gpu_ops.py never reaches (it uses d = 32, 64); route from ops.attention_route

Measured on the MI355X (pytest -s prints one line per row; profiles/attention_route_table.md lists every row beside the CPU emulation):
worst |out - y| / bar 0.004 - 0.016 on unit-amplitude rows, 0.049 on the f16-split q x 8 row, 0.050 on the clamp row, 0 on the one-key
rows; max |out - true| <= 9.1e-7 on unit rows.  The garbage-padding and the strided runs are bit-identical to their plain runs.  No row
found a defect in the kernels.

Mutations (scratch builds, one arithmetic line each, no address computation touched; the table is in profiles/attention_route_table.md):
the mask comparison off by one fails every masked and wrapper row -- in attention_cf_kernel alone 26 rows and in
attention_cf_f16s_kernel<16> alone 15, with all standing attention tests of test_gpu_ops.py passing; a masked key index of another
accumulator layout (r + 16 half) fails nk_valid 37 .. 49 (at 33, 36, 61, 63 it masks the same keys: why the table holds all of them); a
dropped lo term of either product fails 32 - 37 of the 37 f16-split rows; a missing alpha on o or on l fails every row with two key blocks
and alpha < 1; the clamp at 65504 fails the clamp row; inputs read with b and h exchanged fail every B = 2 row.  Exchanging b and h for
inputs and output alike is an equivalent mutant (the output pointer is formed from the same b, h: the workgroups are renumbered)."""
import pytest
import torch

from _attention_refs import (BLOCK_ROWS, CLAMP_ROWS, LONG_ROWS, MASK_ROWS, RESCALE_ROWS, STRIDE_ROWS, WRAPPER_ROWS, garbage_padding, row_refs,
                             worst_ratio)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12345.5                         # the fence around the output
PAD = 64                                # floats of fence on each side: keeps the output 16-byte aligned
KERNEL = {0: "attention_cf_kernel", 1: "attention_cf_f16s_kernel"}

_REFS = {}


def refs_of(row):
    """the row's inputs and references, computed once and modified by nobody"""
    if row.name not in _REFS:
        _REFS[row.name] = row_refs(row)
    return _REFS[row.name]


def fenced(x, dev, lead):
    """a contiguous device copy of x `lead` floats into a buffer with NaNs before and after (4: 16-byte aligned, 1: pointer % 16 == 4)"""
    assert lead in (1, 4)
    buf = torch.full((x.numel() + lead + (4 if lead == 4 else 7),), NAN, device=dev)
    xd = buf[lead:lead + x.numel()].view(x.shape)
    xd.copy_(x.to(dev))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == (4 * lead) % 16
    assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + x.numel():]).all())
    return xd


def v_lead(row):
    return 4 if row.route == 1 else 1


def bs(t):
    """element batch stride of a [B, C, N] tensor or channel slice"""
    assert t.stride(2) == 1 and t.stride(1) == t.shape[2]
    return t.stride(0)


def call(dev, row, qd, kd, vd):
    """probe, then the C ABI into a fenced NaN-filled output -> [B, C, Nq] float32 on the CPU"""
    from cineflow._lib import check, lib
    B, C = row.B, row.heads * row.d
    assert qd.shape == (B, C, row.Nq) and kd.shape == vd.shape == (B, C, row.Nk)
    probe = lib().cf_attention_cf_route(vd.data_ptr(), bs(vd), row.d, row.Nk)
    assert probe == row.route, "%s: the probe names %s<%d>, the row is for %s<%d>" % (row.name, KERNEL.get(probe, probe), row.d, KERNEL[row.route], row.d)
    n = B * C * row.Nq
    buf = torch.full((n + 2 * PAD,), SENT, device=dev)
    out = buf[PAD:PAD + n]
    out.fill_(NAN)
    assert out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    if row.nk_valid < row.Nk:
        check(lib().cf_attention_cf_masked(qd.data_ptr(), bs(qd), kd.data_ptr(), bs(kd), vd.data_ptr(), bs(vd), out.data_ptr(), B, row.heads, row.d,
                                           row.Nq, row.Nk, row.nk_valid, stream), "cf_attention_cf_masked")
    else:
        check(lib().cf_attention_cf(qd.data_ptr(), bs(qd), kd.data_ptr(), bs(kd), vd.data_ptr(), bs(vd), out.data_ptr(), B, row.heads, row.d,
                                    row.Nq, row.Nk, stream), "cf_attention_cf")
    host = buf.cpu()
    assert bool((host[:PAD] == SENT).all()) and bool((host[PAD + n:] == SENT).all()), "%s: the kernel wrote outside its output" % row.name
    return host[PAD:PAD + n].view(B, C, row.Nq)


def run_plain(dev, row, q, k, v):
    return call(dev, row, fenced(q, dev, 1), fenced(k, dev, 1), fenced(v, dev, v_lead(row)))


def judge(row, got, r, tag="", nq=None):
    """the row's bar, and the standing 2e-5 on unit-amplitude rows; nq: compare the first nq queries only (the wrapper's real ones)"""
    y, bar, true = (t if nq is None else t[:, :, :nq] for t in (r["y"], r["bar"], r["true"]))
    assert got.shape == y.shape
    worst = worst_ratio(got, y, bar)
    absd = float((got.double() - true).abs().max())
    print("\n  %-26s %-14s route %d  |out - y| / bar %.4f   max|out - true| %.2e" % (row.name, tag, row.route, worst, absd))
    assert worst <= 1.0, "%s %s: %.3f x its bar (NaN: an element no kernel wrote, or a read outside an input)" % (row.name, tag, worst)
    if row.unit:
        assert absd <= 2e-5, "%s %s: max|out - true| %.3e > 2e-5" % (row.name, tag, absd)
    return worst


def by_name(rows):
    return pytest.mark.parametrize("row", rows, ids=[r.name for r in rows])


@by_name(BLOCK_ROWS + RESCALE_ROWS + LONG_ROWS + CLAMP_ROWS)
def test_rows(dev, row):
    (q, k, v), r = refs_of(row)
    got = run_plain(dev, row, q, k, v)
    assert bool(torch.isfinite(got).all())
    judge(row, got, r)


@by_name(MASK_ROWS)
def test_mask_rows(dev, row):
    """zero padding, then finite garbage in the padded keys: the same bits.  One valid key: the output is that key's V row (fp32 kernel:
    p = 1, l = 1, exactly; f16-split kernel: vh + vl, within 2^-22 |v| + 2^-25 of v, the resolution of the split)"""
    (q, k, v), r = refs_of(row)
    got = run_plain(dev, row, q, k, v)
    judge(row, got, r, "zero padding")
    if row.nk_valid < row.Nk:
        kg, vg = garbage_padding(row, k, v)
        assert not torch.equal(kg, k) and float(vg[:, :, row.nk_valid:].min()) == 1000.0
        again = run_plain(dev, row, q, kg, vg)
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), "%s: the padded keys reach the output (max difference %.3e)" % (
            row.name, float((again - got).abs().max()))
    if row.nk_valid == 1:
        want = v[:, :, :1].expand_as(got)
        if row.route == 0:
            assert torch.equal(got, want)
        else:
            assert bool(((got.double() - want.double()).abs() <= 2.0 ** -22 * want.double().abs() + 2.0 ** -25).all())


@by_name(STRIDE_ROWS)
def test_stride_rows(dev, row):
    (q, k, v), r = refs_of(row)
    B, C, N = q.shape
    assert row.Nq == row.Nk
    plain = run_plain(dev, row, q, k, v)
    judge(row, plain, r, "contiguous")
    qk = fenced(torch.cat([q, k], 1), dev, 1)                       # [B, 2C, N], one float into its fence; V apart
    same_qk = call(dev, row, qk.narrow(1, 0, C), qk.narrow(1, C, C), fenced(v, dev, v_lead(row)))
    judge(row, same_qk, r, "[B, 2C, N] + V")
    qkv = fenced(torch.cat([q, k, v], 1), dev, v_lead(row))         # [B, 3C, N]: V is its last third, so the route decides the offset
    thirds = call(dev, row, qkv.narrow(1, 0, C), qkv.narrow(1, C, C), qkv.narrow(1, 2 * C, C))
    judge(row, thirds, r, "[B, 3C, N]")
    for other, what in ((same_qk, "[B, 2C, N] + V"), (thirds, "[B, 3C, N]")):
        assert torch.equal(other.view(torch.int32), plain.view(torch.int32)), "%s: %s differs from the contiguous call" % (row.name, what)


@by_name(WRAPPER_ROWS)
def test_wrapper_rows(dev, row):
    """ops.attention_cf pads ragged token counts itself and masks the padded keys; the reference is taken on the padded tensors"""
    from cineflow import ops
    (q, k, v), r = refs_of(row)
    nq, nk = int(row.kind.split(":")[1]), row.nk_valid
    qd, kd, vd = (t.contiguous().to(dev) for t in (q[:, :, :nq], k[:, :, :nk], v[:, :, :nk]))
    probe = ops.attention_route(vd, row.heads, nq)
    assert probe == row.route, "%s: the probe names %s, the row is for %s" % (row.name, KERNEL.get(probe, probe), KERNEL[row.route])
    got = ops.attention_cf(qd, kd, vd, row.heads).cpu()
    assert got.shape == (row.B, row.heads * row.d, nq)
    judge(row, got, r, "%d x %d" % (nq, nk), nq=nq)
