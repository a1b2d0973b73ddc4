"""The label maps cf_crop_windows is held to (tests/test_gpu_crop_windows.py) and the numpy restatement of its arithmetic, which
tests/test_mtl_folder_cpu.py holds to Processor.get_mean_centroid + adjust_cropping_window on the same maps."""
import numpy as np

SIZES = ((12, 8), (96, 64), (12, 12), (10, 6))      # (image, crop): the issue's two, crop == image, and a width that is no multiple of 4


def _box(S, x1, x2, y1, y2):
    m = np.zeros((S, S), dtype=np.uint8)
    m[y1:y2 + 1, x1:x2 + 1] = 1
    return m


def cases(S):
    """[(name, uint8 [S,S])]: an empty map, one pixel in each corner (both clamps on both axes), boxes of odd and even width and height
    (the .5 of the centre), a box touching each border, a box that needs no clamp, labels > 1 and scattered pixels"""
    q, h = S // 4, S // 2
    out = [("empty", np.zeros((S, S), dtype=np.uint8))]
    for name, (x, y) in (("corner_tl", (0, 0)), ("corner_tr", (S - 1, 0)), ("corner_bl", (0, S - 1)), ("corner_br", (S - 1, S - 1))):
        out.append((name, _box(S, x, x, y, y)))
    out.append(("even_w_even_h", _box(S, q, q + 3, q + 1, q + 4)))        # x2 - x1 = 3: centre .5
    out.append(("odd_w_odd_h", _box(S, q, q + 4, q + 1, q + 3)))          # x2 - x1 = 4: whole centre
    out.append(("even_w_odd_h", _box(S, h - 1, h + 2, h - 2, h + 2)))
    out.append(("odd_w_even_h", _box(S, h - 2, h + 2, h, h + 1)))
    out.append(("touch_left", _box(S, 0, 2, h - 1, h + 1)))
    out.append(("touch_right", _box(S, S - 3, S - 1, h - 1, h)))
    out.append(("touch_top", _box(S, h - 1, h + 1, 0, 1)))
    out.append(("touch_bottom", _box(S, h, h + 2, S - 2, S - 1)))
    out.append(("centre", _box(S, h - 1, h, h - 1, h)))
    m = np.zeros((S, S), dtype=np.uint8)                                   # two far pixels with other label values: the box spans them
    m[1, S - 2] = 3
    m[S - 3, 2] = 255
    out.append(("scattered", m))
    out.append(("full", np.ones((S, S), dtype=np.uint8)))
    return out


def batch(S, N):
    """N maps: the cases of size S, repeated in order"""
    cs = cases(S)
    return np.stack([cs[i % len(cs)][1] for i in range(N)])


def windows_numpy(lab, crop, image):
    """lab uint8 [N,H,W] -> (windows int32 [N,4] = (x_low, x_high, y_low, y_high), jobs int32 [N,3] = (n, y_low, x_low)): the integer
    arithmetic cf_crop_windows documents"""
    N, H, W = lab.shape
    win, jobs = np.zeros((N, 4), dtype=np.int32), np.zeros((N, 3), dtype=np.int32)
    half = crop // 2
    for n in range(N):
        ys, xs = np.nonzero(lab[n])
        if len(xs) == 0:
            cx, cy = H // 2, W // 2
        else:
            cx, cy = int(xs.min()) + (int(xs.max()) - int(xs.min())) // 2, int(ys.min()) + (int(ys.max()) - int(ys.min())) // 2
        lo, hi = [], []
        for c in (cx, cy):
            low, high = max(0, c - half), min(image, c + half)
            if low == 0:
                high = crop
            if high == image:
                low = image - crop
            lo.append(low)
            hi.append(high)
        win[n] = (lo[0], hi[0], lo[1], hi[1])
        jobs[n] = (n, lo[1], lo[0])
    return win, jobs
