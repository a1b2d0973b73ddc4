"""The SegFlowGaussian recurrence encodes only what a later step consumes: no memory-encoder pass behind the last step, a pass on the
sequences that go on behind the last common step of two ragged half sequences, and ONE pass over the ED frame both halves of a slice share
(SegFlowGaussian.forward, shared_first) -- with the flow of predict_cine_slices unchanged against plain per-half-sequence calls.

Bound: the schedule-equivalence limits of tests/test_gpu_models.py (test_config4_full_size_one_call): mean EPE <= 2e-5 px and worst pixel
<= 2e-3 px between two schedules of the same network -- the batch size picks the launch shapes and the order of the statistics atomics."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class Counting:
    """an encoder that notes the batch size of every call"""

    def __init__(self, inner):
        self.inner, self.batches = inner, []

    def __call__(self, x):
        self.batches.append(int(x.shape[0]))
        return self.inner(x)


@pytest.mark.parametrize("Tn", [5, 6])
@pytest.mark.parametrize("ma", [False, True])
def test_recurrence_encodes_only_what_is_consumed(dev, ma, Tn):
    from cineflow.models import SegFlowGaussian, Generic_UNet
    from cineflow import inference
    from cineflow.weights import seeded_state_dict
    kw = dict(image_size=64, in_dims=[6, 16, 32], out_encoder_dims=[8, 16, 32], d_model=32, bottleneck_heads=4, dim_feedforward=48, motion_appearance=ma)
    fnet, snet = SegFlowGaussian(**kw), Generic_UNet(1, 8, 4, 3)
    fnet.load_state_dict(seeded_state_dict(fnet.state_shapes(), 21), dev)
    snet.load_state_dict(seeded_state_dict(snet.state_shapes(), 20), dev)
    n = 2
    frames = torch.randn(Tn, n, 1, 64, 64, generator=torch.Generator().manual_seed(102)).to(dev)
    o1, o2 = inference.chunk_orders(Tn)
    mem_enc, qry_enc = fnet.memory_encoder, fnet.query_encoder
    mem, qry = Counting(mem_enc), Counting(qry_enc)
    fnet.memory_encoder, fnet.query_encoder = mem, qry
    try:
        flow = inference.predict_cine_slices(fnet, snet, frames)["flow"]
    finally:
        fnet.memory_encoder, fnet.query_encoder = mem_enc, qry_enc
    steps = len(o1) - 1
    if Tn == 5:
        # equal halves, 3 frames each: the ED frame once for the n slices, every other call on both halves; a memory pass behind each step but the last
        assert len(o1) == len(o2) == 3
        assert mem.batches == [n] + [2 * n] * (steps - 1)
        assert qry.batches == [n] + [2 * n] * steps
    else:
        # ragged halves, 4 and 3 frames: steps 1, 2 on both halves, step 3 on the longer one.  Memory passes: ED (n), behind step 1 (2n), behind
        # step 2 for the half that goes on (n), none behind step 3.  Query passes: ED (n), steps 1, 2 (2n), step 3 (n).
        assert (len(o1), len(o2)) == (4, 3) and steps == 3
        assert mem.batches == [n, 2 * n, n]
        assert qry.batches == [n, 2 * n, 2 * n, n]
    assert len(mem.batches) == steps and len(qry.batches) == steps + 1
    # the same network, one plain forward per half sequence
    ref = torch.zeros_like(flow)
    for order in (o1, o2):
        bf = fnet(frames[order].contiguous())["backward_flow"]
        for j, t in enumerate(order[1:]):
            ref[t] = bf[j]
    dm = float(torch.sqrt(((flow - ref) ** 2).sum(2)).mean())
    d = float((flow - ref).abs().max())
    print("\nma=%s T=%d: predict_cine_slices vs per-half forward: mean EPE %.2e px (bar 2e-5), max |diff| %.2e px (bar 2e-3); |flow| mean %.3f"
          % (ma, Tn, dm, d, float(ref.abs().mean())))
    assert float(ref.abs().mean()) > 1e-3
    assert dm <= 2e-5 and d <= 2e-3
