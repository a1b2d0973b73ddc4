"""cf_crop_windows: Processor.get_mean_centroid of one frame + Processor.adjust_cropping_window per sample on the device, integer for
integer against the host Processor path (cineflow.inference.Processor, whose boxes come from cf_frame_boxes and whose arithmetic is the
reference's, and the oracle's Processor on the CPU); the job table it writes makes cf_tile_gather cut Processor.crop_and_pad's crops."""
import numpy as np
import pytest
import torch

from _crop_window_cases import SIZES, batch, cases, windows_numpy

pytestmark = pytest.mark.gpu


def _host_windows(lab, crop, image, dev):
    """per sample: cineflow's Processor on the device map and the oracle's on the CPU map must agree; -> int32 [N,4]"""
    from cineflow.inference import Processor
    from oracle import models as OM
    mine, ora = Processor(crop, image), OM.Processor(crop, image)
    out = []
    for n in range(lab.shape[0]):
        a = mine.adjust_cropping_window(mine.get_mean_centroid(torch.from_numpy(lab[n:n + 1]).to(dev)))["crop_indices"]
        b = ora.adjust_cropping_window(ora.get_mean_centroid(torch.from_numpy(lab[n:n + 1]).long()))["crop_indices"]
        assert list(a) == list(b), (n, a, b)
        out.append(a)
    return np.asarray(out, dtype=np.int32)


@pytest.mark.parametrize("image,crop", SIZES)
def test_crop_windows_equal_the_host_processor_case_by_case(dev, image, crop):
    """N = 1: every case on its own"""
    from cineflow import ops
    for name, m in cases(image):
        lab = m[None]
        win, jobs = ops.crop_windows(torch.from_numpy(lab).to(dev), crop, image)
        want = _host_windows(lab, crop, image, dev)
        assert np.array_equal(win.cpu().numpy(), want), (name, win.cpu().numpy(), want)
        assert jobs.cpu().numpy().tolist() == [[0, int(want[0, 2]), int(want[0, 0])]], name
        assert np.array_equal(want, windows_numpy(lab, crop, image)[0]), name


@pytest.mark.parametrize("image,crop", SIZES)
def test_crop_windows_batch_of_70_and_the_gather_it_feeds(dev, image, crop):
    """N = 70: one block per sample, 70 blocks; the windows are those of the per-sample host path and cf_tile_gather with the job table
    cuts exactly Processor.crop_and_pad's crops"""
    from cineflow import ops
    from cineflow.inference import Processor
    N = 70
    lab = batch(image, N)
    win, jobs = ops.crop_windows(torch.from_numpy(lab).to(dev), crop, image)
    want = _host_windows(lab, crop, image, dev)
    assert np.array_equal(win.cpu().numpy(), want)
    wn, jn = windows_numpy(lab, crop, image)
    assert np.array_equal(win.cpu().numpy(), wn) and np.array_equal(jobs.cpu().numpy(), jn)
    x = torch.randn(N, 1, image, image, generator=torch.Generator().manual_seed(3)).to(dev)
    got = ops.tile_gather(x, jobs, crop, crop)
    proc = Processor(crop, image)
    for n in (0, 1, 4, 9, 33, 69):
        c, _pad = proc.crop_and_pad(x[n][None].contiguous(), [int(want[n, 0]) + crop // 2, int(want[n, 2]) + crop // 2])
        assert torch.equal(got[n], c[0]), n


def test_crop_windows_second_grid_trip(dev):
    """more samples than the grid's 4096 blocks: the tail is served by a second trip of the first blocks"""
    from cineflow import ops
    N = 4096 + 40
    lab = batch(12, N)
    win, jobs = ops.crop_windows(torch.from_numpy(lab).to(dev), 8, 12)
    wn, jn = windows_numpy(lab, 8, 12)
    assert np.array_equal(win.cpu().numpy(), wn) and np.array_equal(jobs.cpu().numpy(), jn)
