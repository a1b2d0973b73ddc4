"""cf_window_attention on its own, against the fp64 restatement of the Swin windowed cross-attention (tests/_kernel_refs.py, pinned to
oracle.mtl's CrossAttention under its own attn_mask and relative_position_index buffers in test_kernel_refs_cpu.py).  The product
reaches the kernel only inside SwinFilterBlock behind seeded projections at ws 8 / hd 8 and ws 7 / hd 4; this table adds H != W, shifts
other than ws / 2, more than 4 heads, a head dimension that is no power of two, and ws 8 / hd 64 -- the one launch that needs 66,560
bytes of dynamic LDS and with it the opt-in above 64 KB.

Bars: 2e-5 on randn inputs and 5e-4 with q and k scaled x30, the attention tests' bars (test_gpu_ops.py); a constant v in (0, 1] comes
back at 1e-5 (a softmax row of N <= 64 fp32 terms sums to 1 within N * 2^-24 = 4e-6, and the error scales with |v|).  The shifted rows are rerun against the restatement WITHOUT its -100 mask term and must then miss the bar: the bar resolves the mask.

Measured on the MI355X (pytest -s; max|diff|, ratio to the bar):
  B heads hd  H  W ws shift    table          constant v      mask left out    q, k x30
  2   2    8 32 32  8   4   6.04e-7 0.030   6.56e-7 0.066      1.22           2.14e-4 0.43
  1   2    4 28 28  7   3   5.74e-7 0.029   4.17e-7 0.042      1.41
  2   4   32 14 28  7   3   8.86e-7 0.044   5.96e-7 0.060      1.88           3.80e-4 0.76
  1   1   16  8 24  4   0   3.68e-7 0.018   2.98e-7 0.030       -
  1   8    8 16  8  8   1   1.23e-6 0.062   7.75e-7 0.077      3.17
  2   3    5  6  4  2   1   2.85e-7 0.014   1.19e-7 0.012      3.49
  1   2   64 16 16  8   4   9.75e-7 0.049   6.56e-7 0.066      1.60           2.25e-4 0.45
"""
import pytest
import torch

from _kernel_refs import ratio_line, window_attention

pytestmark = pytest.mark.gpu

#        B  heads hd   H   W  ws shift
TABLE = [(2, 2, 8, 32, 32, 8, 4),
         (1, 2, 4, 28, 28, 7, 3),
         (2, 4, 32, 14, 28, 7, 3),          # H != W
         (1, 1, 16, 8, 24, 4, 0),
         (1, 8, 8, 16, 8, 8, 1),            # shift != ws / 2, W == ws: one window column holding all three border regions
         (2, 3, 5, 6, 4, 2, 1),
         (1, 2, 64, 16, 16, 8, 4)]          # the > 64 KB LDS launch


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max())


def _inputs(row, scale=1.0):
    B, heads, hd, H, W, ws, shift = row
    C = heads * hd
    seed = 1000 * ws + 10 * hd + shift
    q, k, v = scale * randn(B, C, H, W, seed=seed), scale * randn(B, C, H, W, seed=seed + 1), randn(B, C, H, W, seed=seed + 2)
    return q, k, v, 0.5 * randn((2 * ws - 1) ** 2, heads, seed=seed + 3)


def _run(dev, row, q, k, v, table):
    from cineflow import ops
    B, heads, hd, H, W, ws, shift = row
    out = ops.window_attention(torch.cat([q, k], 1).contiguous().to(dev), v.to(dev), table.to(dev), heads, ws, shift)
    assert tuple(out.shape) == tuple(v.shape)
    return out


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "B%d-h%d-hd%d-%dx%d-ws%d-s%d" % r)
def test_window_attention_table(dev, row):
    B, heads, hd, H, W, ws, shift = row
    q, k, v, table = _inputs(row)
    out = _run(dev, row, q, k, v, table)
    worst = maxdiff(out, window_attention(q, k, v, table, heads, ws, shift))
    print()
    ratio_line("window_attention %s" % (row,), worst, 2e-5)
    assert worst <= 2e-5
    if shift > 0:                                                        # without the -100 term the same run misses the bar
        blind = maxdiff(out, window_attention(q, k, v, table, heads, ws, shift, mask=False))
        ratio_line("window_attention %s, mask left out of the reference" % (row,), blind, 2e-5)
        assert blind > 2e-5
    C = heads * hd                                                       # one value per channel in (0, 1]: the bar is absolute, the error scales with |v|
    const = (torch.arange(1, C + 1, dtype=torch.float32) / C).view(1, -1, 1, 1).expand(B, -1, H, W).contiguous()
    back = maxdiff(_run(dev, row, q, k, const, table), const)
    ratio_line("window_attention %s, constant v" % (row,), back, 1e-5)
    assert back <= 1e-5


@pytest.mark.parametrize("row", [TABLE[0], TABLE[2], TABLE[6]], ids=lambda r: "B%d-h%d-hd%d-%dx%d-ws%d-s%d" % r)
def test_window_attention_large_logits(dev, row):
    B, heads, hd, H, W, ws, shift = row
    q, k, v, table = _inputs(row, scale=30.0)                            # q and k x30 each, as the attention tests scale theirs
    worst = maxdiff(_run(dev, row, q, k, v, table), window_attention(q, k, v, table, heads, ws, shift))
    print()
    ratio_line("window_attention %s, q and k x30" % (row,), worst, 5e-4)
    assert worst <= 5e-4


def test_window_attention_host_checks(dev):
    from cineflow import ops
    from cineflow._lib import CineflowError

    from cineflow._lib import check, lib

    def call(heads, hd, H, W, ws, shift):
        C = heads * hd
        qk, v = torch.zeros(1, 2 * C, H, W, device=dev), torch.full((1, C, H, W), -7.0, device=dev)
        tbl = torch.zeros((2 * abs(ws) - 1) ** 2, heads, device=dev)
        out = torch.full((1, C, H, W), 3.0, device=dev)
        check(lib().cf_window_attention(qk.data_ptr(), v.data_ptr(), tbl.data_ptr(), out.data_ptr(), 1, C, H, W, heads, ws, shift,
                                        torch.cuda.current_stream().cuda_stream), "cf_window_attention")
        return out

    for bad in ((2, 4, 18, 18, 9, 0), (2, 4, 12, 16, 8, 0), (2, 4, 16, 12, 8, 0), (2, 4, 16, 16, 8, 8), (2, 4, 16, 16, 8, -1), (1, 65, 8, 8, 8, 0)):
        with pytest.raises(CineflowError):                               # window 9, a window not dividing H or W, shift == window, hd > 64
            call(*bad)
    good = call(2, 4, 16, 16, 8, 0)                                      # and a good call runs: zero logits average a constant v
    assert float((good + 7.0).abs().max()) <= 1e-5
    with pytest.raises(AssertionError):
        ops.window_attention(torch.zeros(1, 16, 16, 16, device=dev), torch.zeros(1, 8, 16, 16, device=dev), torch.zeros(49, 2, device=dev), 2, 8, 0)
