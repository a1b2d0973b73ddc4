"""cf_cine_ssim_table (csrc/score.hip) through cineflow.metrics.ssim_sums_table / cine_ssim_table against the fp64 oracle, decomposed so
that no new tolerance is needed:
  * the registered images the table scored equal ops.warp_bilinear on the same inputs bit for bit (the same kernel, which
    tests/test_gpu_ops.py ties to the oracle);
  * every (frame, slice) is compared with oracle.metrics.structural_similarity(fixed[d], registered_dev[t, d], data_range=max - min,
    full=True) on the device's own registered image: the interior mean within 1e-10, every structure's mean within 1e-9 (the score and map
    bars of tests/test_metrics.py and tests/test_gpu_metrics_kernels.py), NaN meeting NaN, counts exact.  The separable row-then-column
    summation differs from scipy's uniform_filter by rounding alone: measured on an MI355X at most 5.1e-14 (interior means) and 3.7e-14
    (structure means) over these cases.
Shapes: a one-pixel interior with reflection on every side (7x7/7, 15x15/15), exactly one tile (32x64), a 1-pixel second tile in both
directions (33x65), and windows 3, 11 on maps that are no multiple of the tile; (T, D) = (1, 1) and (3, 2)."""
import numpy as np
import pytest
import torch

from _kernel_refs import ratio_line
from _score_refs import smooth_flow, structure_labels
from oracle import metrics as OM

pytestmark = pytest.mark.gpu

WHOLE_BAR, STRUCT_BAR = 1e-10, 1e-9
SHAPES = [(7, 7, 7), (32, 64, 7), (33, 65, 7), (40, 70, 11), (9, 130, 3), (15, 15, 15)]
NAMES = ("RV", "MYO", "LV")


def make_cine(seed, T, D, H, W, scale=1.0):
    """fixed [H, W, D] ~ N(300, 40^2), moving [T, H, W, D] = fixed + N(0, 10^2), flow [T, H, W, D, 2] of amplitude 1.6"""
    rng = np.random.default_rng(seed)
    fixed = rng.normal(300.0, 40.0, size=(H, W, D)) * scale
    moving = ((fixed[None] + rng.normal(0.0, 10.0, size=(T, H, W, D)) * scale)).astype(np.float32)
    return rng, fixed, moving, smooth_flow(rng, T, H, W, D, 1.6)


def oracle_slice(fixed, reg, t, d, win):
    r = reg[t, :, :, d]
    return OM.structural_similarity(fixed[:, :, d], r, data_range=float(r.max() - r.min()), win_size=win, full=True)


def check_against_oracle(tag, fixed, reg, labels, win, tab, rows, K):
    """tab [T, D, 2 + 2 K] and the rows of cine_ssim_table against the oracle on the registered images `reg` [T, H, W, D]; returns the
    worst (whole, structure) differences"""
    T, D = tab.shape[:2]
    H, W = fixed.shape[:2]
    pad = (win - 1) // 2
    worst_w = worst_s = 0.0
    assert len(rows) == T * D
    for d in range(D):
        for t in range(T):
            with np.errstate(invalid="ignore", divide="ignore"):
                want, wmap = oracle_slice(fixed, reg, t, d, win)
            row = rows[d * T + t]
            assert tab[t, d, 1] == (H - 2 * pad) * (W - 2 * pad), (tag, t, d, tab[t, d, 1])
            got = row["SSIM_whole"]
            if np.isnan(want):
                assert np.isnan(got), (tag, t, d, got)
            else:
                assert not np.isnan(got), (tag, t, d)
                worst_w = max(worst_w, abs(got - want))
            if labels is None:
                assert set(row) == {"SSIM_whole"}
                continue
            per = []
            for k in range(K):
                sel = labels[:, :, d] == k
                assert tab[t, d, 3 + 2 * k] == sel.sum(), (tag, t, d, k, tab[t, d, 3 + 2 * k], sel.sum())
                if k == 0:
                    continue
                got = row["SSIM_" + NAMES[k - 1].lower()]
                per.append(got)
                if not sel.any():
                    assert np.isnan(got) and tab[t, d, 2 + 2 * k] == 0.0, (tag, t, d, k, got)
                    continue
                with np.errstate(invalid="ignore"):
                    w = wmap[sel].mean()
                if np.isnan(w):
                    assert np.isnan(got), (tag, t, d, k, got)
                else:
                    assert not np.isnan(got), (tag, t, d, k)
                    worst_s = max(worst_s, abs(got - w))
            mean = row["SSIM_mean"]
            assert (np.isnan(mean) and np.isnan(sum(per))) or mean == sum(per) / 3
    return worst_w, worst_s


def score(fixed, moving, flow, labels, win, **kw):
    """-> (tab, rows, registered [T, H, W, D] numpy): the raw table of one call, the rows and the registered images of another; the two calls
    must agree bit for bit"""
    from cineflow import metrics
    K = 4 if labels is not None else 0
    tab, reg_dev = metrics.ssim_sums_table(fixed, moving, flow, labels, K, win, **kw)
    rows, reg = metrics.cine_ssim_table(fixed, moving, flow, labels, NAMES, win, return_registered=True, **kw)
    assert np.array_equal(reg_dev.permute(0, 2, 3, 1).cpu().numpy(), reg)
    tab2, _ = metrics.ssim_sums_table(fixed, moving, flow, labels, K, win, **kw)
    assert tab.tobytes() == tab2.tobytes(), "two calls must give the same bits"
    with np.errstate(invalid="ignore", divide="ignore"):
        whole = tab[:, :, 0] / tab[:, :, 1]
    assert np.array_equal(whole.T.reshape(-1), np.array([r["SSIM_whole"] for r in rows]), equal_nan=True)
    return tab, rows, reg


def device_warp(dev, moving, flow):
    """ops.warp_bilinear frame by frame (B = D) -> [T, H, W, D]"""
    from cineflow import ops
    out = []
    for t in range(moving.shape[0]):
        f = torch.from_numpy(flow[t]).to(dev).permute(2, 3, 0, 1).contiguous()
        m = torch.from_numpy(moving[t]).to(dev).permute(2, 0, 1)[:, None].contiguous()
        out.append(ops.warp_bilinear(f, m)[:, 0].permute(1, 2, 0).cpu().numpy())
    return np.stack(out)


@pytest.mark.parametrize("T,D", [(1, 1), (3, 2)])
@pytest.mark.parametrize("H,W,win", SHAPES)
def test_table_matches_the_oracle(dev, H, W, win, T, D):
    scale = 10.0 if (H, W, T) == (40, 70, 3) else 1.0
    rng, fixed, moving, flow = make_cine(H * 1000 + W * 10 + T, T, D, H, W, scale)
    labels = structure_labels(rng, (H, W, D))
    tab, rows, reg = score(fixed, moving, flow, labels, win)
    assert reg.dtype == np.float32 and reg.tobytes() == device_warp(dev, moving, flow).tobytes(), "the registered images are ops.warp_bilinear's"
    tag = "cine_ssim_table %dx%d win %d T=%d D=%d" % (H, W, win, T, D)
    ww, ws = check_against_oracle(tag, fixed, reg, labels, win, tab, rows, 4)
    print()
    assert ratio_line(tag + " whole", ww, WHOLE_BAR) <= 1 and ratio_line(tag + " structures", ws, STRUCT_BAR) <= 1


def test_label_cases(dev):
    H, W, D, T, win = 33, 65, 3, 2, 7
    rng, fixed, moving, flow = make_cine(5, T, D, H, W)
    labels = structure_labels(rng, (H, W, D))
    labels[:, :, 0][labels[:, :, 0] == 2] = 0                     # MYO absent from slice 0: NaN mean, count 0
    labels[:, :, 1][labels[:, :, 1] == 1] = 0                     # RV of slice 1 wholly in the border band outside the interior
    labels[:2, :, 1] = 1
    labels[H - 1, W - 3:, 1] = 1
    labels[10:14, 20:30, 2] = 7                                   # a label >= K counts nowhere
    tab, rows, reg = score(fixed, moving, flow, labels, win)
    ww, ws = check_against_oracle("labels", fixed, reg, labels, win, tab, rows, 4)
    assert np.isnan(rows[0]["SSIM_myo"]) and np.isnan(rows[0]["SSIM_mean"]) and not np.isnan(rows[T]["SSIM_mean"])
    assert tab[0, 1, 3 + 2 * 1] == 2 * W + 3
    assert tab[0, 2, 3::2].sum() == H * W - 40 and tab[0, 0, 3::2].sum() == H * W
    print()
    assert ratio_line("label cases whole", ww, WHOLE_BAR) <= 1 and ratio_line("label cases structures", ws, STRUCT_BAR) <= 1
    # labels=None: the whole-slice columns alone, the same bits
    tab0, rows0, _ = score(fixed, moving, flow, None, win)
    assert tab0.shape == (T, D, 2) and tab0.tobytes() == np.ascontiguousarray(tab[:, :, :2]).tobytes()
    # int64 labels: values outside [0, K) count nowhere either
    from cineflow import metrics
    tab64, _ = metrics.ssim_sums_table(fixed, moving, flow, labels.astype(np.int64), 4, win)
    assert tab64.tobytes() == tab.tobytes()


def test_special_slices(dev):
    H, W, D, T, win = 40, 70, 4, 2, 7
    rng, fixed, moving, flow = make_cine(6, T, D, H, W)
    labels = structure_labels(rng, (H, W, D))
    fixed[:, :, 1] = 0.0                                          # fixed and registered both all zero: R = 0, S = 0 / 0
    moving[:, :, :, 1] = 0.0
    flow[:, :, :, 2] = 1000.0                                     # every tap outside: registered = 0 against a non-constant fixed
    tab, rows, reg = score(fixed, moving, flow, labels, win)
    assert not reg[:, :, :, 1].any() and not reg[:, :, :, 2].any()
    ww, ws = check_against_oracle("special", fixed, reg, labels, win, tab, rows, 4)
    for t in range(T):
        assert np.isnan(tab[t, 1, 0::2]).all() and all(np.isnan(v) for v in rows[1 * T + t].values())
        assert not tab[t, 2, 0::2].any() and all(v == 0.0 for v in rows[2 * T + t].values())
        with np.errstate(invalid="ignore", divide="ignore"):
            assert not oracle_slice(fixed, reg, t, 2, win)[1].any()
        assert all(np.isfinite(v) for d in (0, 3) for v in rows[d * T + t].values())
    print()
    assert ratio_line("special slices whole", ww, WHOLE_BAR) <= 1 and ratio_line("special slices structures", ws, STRUCT_BAR) <= 1


def test_registered_branch_gives_the_same_table(dev):
    H, W, D, T, win = 33, 65, 2, 3, 7
    rng, fixed, moving, flow = make_cine(7, T, D, H, W)
    labels = structure_labels(rng, (H, W, D))
    tab, rows, reg = score(fixed, moving, flow, labels, win)
    tab_r, rows_r, reg_r = score(fixed, None, None, labels, win, registered=reg)
    assert tab_r.tobytes() == tab.tobytes() and rows_r == rows and reg_r.tobytes() == reg.tobytes()
    from cineflow import metrics
    rows_t, reg_t = metrics.cine_ssim_table(torch.from_numpy(fixed).to(dev), None, None, torch.from_numpy(labels).to(dev), NAMES, win,
                                            registered=torch.from_numpy(reg).to(dev), return_registered=True)
    assert torch.is_tensor(reg_t) and rows_t == rows


def test_refusals(dev):
    from cineflow import metrics
    from cineflow._lib import CineflowError
    rng, fixed, moving, flow = make_cine(8, 1, 1, 20, 20)
    labels = structure_labels(rng, (20, 20, 1))
    for win in (6, 17, 21):
        with pytest.raises(CineflowError, match="win"):
            metrics.cine_ssim_table(fixed, moving, flow, labels, win_size=win)
    with pytest.raises(CineflowError, match="win=9 exceeds"):
        metrics.cine_ssim_table(fixed[:7, :9], moving[:, :7, :9], flow[:, :7, :9], win_size=9)
    with pytest.raises(CineflowError, match="K must be"):
        metrics.cine_ssim_table(fixed, moving, flow, labels, names=tuple("s%d" % i for i in range(16)))
    with pytest.raises(CineflowError, match="T \\* D = 65536"):
        metrics.cine_ssim_table(np.zeros((7, 7, 1)), None, None, registered=torch.zeros((65536, 7, 7, 1), device=dev))
    torch.cuda.synchronize()
