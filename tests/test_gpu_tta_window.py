"""cf_tta_accumulate_window: the flip-TTA softmax of crops accumulated straight into each sample's window of an image-sized buffer, bit
for bit what cf_tta_accumulate into a crop-sized buffer followed by ops.pad2d (Processor.uncrop_no_registration) gives, and nothing
outside the windows touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGE = 12
FLIPS = ((0, 0), (0, 1), (1, 0), (1, 1))
# (x_low, y_low) of three samples per crop size: a corner, the opposite corner region and an interior window, all different
ORIGINS = {8: ((0, 0), (4, 1), (2, 4)), 6: ((6, 6), (0, 3), (1, 0))}


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("crop", (8, 6))
@pytest.mark.parametrize("K", (2, 4))
@pytest.mark.parametrize("folds", (1, 2))
def test_window_accumulate_is_bitwise_crop_accumulate_then_pad(dev, crop, K, folds):
    """weight 1 / (4 * folds) = 1/4 and 1/8: one or two folds' four flips accumulated in sequence into one buffer"""
    from cineflow import ops
    B = 3
    g = torch.Generator().manual_seed(100 * crop + 10 * K + folds)
    win = torch.tensor([[x, x + crop, y, y + crop] for x, y in ORIGINS[crop]], dtype=torch.int32).to(dev)
    logits = [(torch.randn(B, K, crop, crop, generator=g) * 3).to(dev) for _ in range(folds * len(FLIPS))]
    w = 1.0 / (len(FLIPS) * folds)
    pre = (torch.randn(B, K, IMAGE, IMAGE, generator=g) + 2.0).to(dev)      # a second buffer that is not zero anywhere that matters
    assert float(pre.abs().min()) > 0
    acc0, acc1 = torch.zeros(B, K, IMAGE, IMAGE, device=dev), pre.clone()
    ref0 = torch.zeros(B, K, crop, crop, device=dev)
    ref1 = torch.stack([pre[b, :, y:y + crop, x:x + crop] for b, (x, y) in enumerate(ORIGINS[crop])]).contiguous()
    i = 0
    for _f in range(folds):
        for fh, fw in FLIPS:
            ops.tta_accumulate_window(logits[i], win, acc0, fh, fw, w)
            ops.tta_accumulate_window(logits[i], win, acc1, fh, fw, w)
            ops.tta_accumulate(logits[i], ref0, fh, fw, w)
            ops.tta_accumulate(logits[i], ref1, fh, fw, w)
            i += 1
    inside = torch.zeros(B, 1, IMAGE, IMAGE, dtype=torch.bool, device=dev)
    for b, (x, y) in enumerate(ORIGINS[crop]):
        want = ops.pad2d(ref0[b].contiguous(), y, x, IMAGE, IMAGE)          # uncrop_no_registration: rows from y_low, columns from x_low
        assert torch.equal(_bits(acc0[b]), _bits(want)), (b, float((acc0[b] - want).abs().max()))
        inside[b, :, y:y + crop, x:x + crop] = True
        assert torch.equal(_bits(acc1[b, :, y:y + crop, x:x + crop]), _bits(ref1[b])), b
    inside = inside.expand(B, K, IMAGE, IMAGE)
    assert int(inside.sum()) == B * K * crop * crop
    assert torch.equal(_bits(acc1)[~inside], _bits(pre)[~inside]), "an element outside the windows changed"
    assert not torch.equal(_bits(acc1)[inside], _bits(pre)[inside])
    assert float(acc0.sum()) == pytest.approx(B * crop * crop, rel=1e-5)     # every flip's softmax sums to 1 over K, the weights to 1


def test_window_accumulate_skips_a_window_that_leaves_the_map(dev):
    """the table is device data: a window outside the map writes nothing"""
    from cineflow import ops
    win = torch.tensor([[5, 13, 0, 8], [0, 8, -1, 7], [4, 12, 4, 12]], dtype=torch.int32).to(dev)
    acc = torch.zeros(3, 2, IMAGE, IMAGE, device=dev)
    ops.tta_accumulate_window(torch.randn(3, 2, 8, 8).to(dev), win, acc, 0, 0, 1.0)
    assert float(acc[:2].abs().max()) == 0.0 and float(acc[2, :, 4:, 4:].min()) > 0.0 and float(acc[2, :, :4].abs().max()) == 0.0
