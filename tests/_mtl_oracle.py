"""The oracle's statement of MTLmodel's inference wrapper (MTL_model.py:816-936) and of the tiled prediction around it, shared by
tests/test_gpu_mtl_segmenter.py and tests/test_gpu_mtl_folder.py: per sample, on the CPU, from oracle.mtl.MTLmodel, oracle.models.Processor
and oracle.models.mirror_and_predict_2d."""
import numpy as np
import torch
import torch.nn.functional as F

RED = dict(in_dims=[1, 16, 32], out_encoder_dims=[8, 16, 32], conv_depth=[2, 2, 2], spatial_cross_attention_num_heads=[2, 2, 4], bottleneck_heads=8)
IMAGE, CROP, WINDOW = 96, 64, 8


def smooth_images(B, H, W, seed, amp=1.0, base=0.0, noise=0.1):
    """[B,1,H,W]: a 6 x 6 normal field enlarged bicubically plus a little pixel noise -- structure for the cropper to find.  Unit scale,
    as the preprocessed (z-scored) data the sliding window hands the network: at raw intensities (60 +- 20) the seeded segmenter's logits
    reach 330 and the float32 oracle itself is 3.8e-5 from its float64 run, which leaves a 5e-5 bound no room; at unit scale the logits
    stay below 8 and the oracle's own float32 error is 5e-7."""
    g = torch.Generator().manual_seed(seed)
    x = F.interpolate(torch.randn(B, 1, 6, 6, generator=g), size=(H, W), mode="bicubic", align_corners=False) * amp + base
    return x + noise * torch.randn(B, 1, H, W, generator=g)


def oracle_nets(crop_seed, seg_seeds, dtype=torch.float32):
    from cineflow.weights import fill_module_
    from oracle import mtl as OMTL
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        crop = fill_module_(OMTL.MTLmodel(IMAGE, WINDOW, 2, **RED), crop_seed).eval().to(dtype)
        segs = [fill_module_(OMTL.MTLmodel(CROP, WINDOW, 4, **RED), s).eval().to(dtype) for s in seg_seeds]
    finally:
        torch.set_default_dtype(prev)
    return crop, segs


class _Logits:
    def __init__(self, net, num_classes):
        self.net, self.num_classes = net, num_classes

    def __call__(self, x):
        p = next(self.net.parameters())
        return self.net(x.to(p.dtype))["pred"].float()


def cropper_logits(ocrop, x):
    """the logits Processor.discretize's argmax is taken from, per sample ([1,2,H,W], or None for an all-zero sample)"""
    from oracle import ops as OO
    out = []
    p = next(ocrop.parameters())
    with torch.no_grad():
        for b in range(x.shape[0]):
            cur = x[b][None].to(p.dtype)
            out.append(None if torch.count_nonzero(cur) == 0 else ocrop(OO.normalize_intensity(cur))["pred"])
    return out


def top_two_gap(logits):
    top = logits.sort(dim=1, descending=True)[0]
    return top[:, 0] - top[:, 1]


def oracle_wrapper(ocrop, oseg, x, normalize, do_mirroring=True):
    """x [B,1,IMAGE,IMAGE] -> (softmax [B,4,IMAGE,IMAGE], windows [B][4]): crop around the cropper's centroid, optional z-score, flip TTA
    on the crop, zero-pad back -- sample by sample.  oseg: one network, or a list (the folds: the mean of their softmax; the cropper is
    one fixed network and its window serves them all)"""
    from oracle import models as OM
    from oracle import ops as OO
    osegs = list(oseg) if isinstance(oseg, (list, tuple)) else [oseg]
    proc = OM.Processor(CROP, IMAGE, _Dict(ocrop))
    out, wins = [], []
    with torch.no_grad():
        for b in range(x.shape[0]):
            cen, _ = proc.preprocess_no_registration(x[b][None].clone())
            wins.append(list(proc.adjust_cropping_window(cen)["crop_indices"]))
            c, pn = proc.crop_and_pad(x[b][None], cen)
            if normalize:
                c = OO.normalize_intensity(c[0])[None]
            p = sum(OM.mirror_and_predict_2d(_Logits(o, 4), c, (0, 1), do_mirroring) for o in osegs) / len(osegs)
            out.append(proc.uncrop_no_registration(p, pn[None])[0])
    return torch.stack(out), wins


class _Dict:
    """a cropper of any dtype behind Processor.discretize's interface (float32 in, {'pred': float32 logits} out)"""

    def __init__(self, net):
        self.net = net

    def __call__(self, x):
        p = next(self.net.parameters())
        return {"pred": self.net(x.to(p.dtype))["pred"].float()}


def oracle_tiled(ocrop, osegs, data, normalize=False, step_size=0.5):
    """oracle.models.predict_3d_2dconv_tiled with the wrapper above as the tile network and the fold mean: data numpy [1,Z,X,Y] ->
    softmax [4,Z,X,Y] float32 (neural_network.py:623-769 tile order, Gaussian weighting when there is more than one tile)"""
    from oracle import ops as OO
    patch = (IMAGE, IMAGE)
    probs = []
    for z in range(data.shape[1]):
        d, slicer = OO.pad_nd_image(data[:, z], patch, "constant", {"constant_values": 0}, True, None)
        steps = OO.compute_steps_for_sliding_window(patch, d.shape[1:], step_size)
        many = len(steps[0]) * len(steps[1]) > 1
        g = OO.get_gaussian(patch, sigma_scale=1.0 / 8) if many else np.ones(patch, dtype=np.float32)
        agg = np.zeros((4,) + d.shape[1:], dtype=np.float32)
        cnt = np.zeros((4,) + d.shape[1:], dtype=np.float32)
        for lx in steps[0]:
            for ly in steps[1]:
                tile = torch.from_numpy(np.ascontiguousarray(d[None, :, lx:lx + IMAGE, ly:ly + IMAGE])).float()
                pred = oracle_wrapper(ocrop, osegs, tile, normalize)[0]
                agg[:, lx:lx + IMAGE, ly:ly + IMAGE] += pred[0].numpy() * (g if many else 1.0)
                cnt[:, lx:lx + IMAGE, ly:ly + IMAGE] += g
        sl = (slice(None),) + tuple(slicer[1:])
        probs.append((agg / cnt)[sl])
    return np.stack(probs, 1)


def patient_volumes(Y, X, seed, frames=2, slices=3):
    """[frames, slices, Y, X] float32 intensities around 100 +- 40 with structure (smooth_images) for the files of a synthetic patient"""
    return smooth_images(frames * slices, Y, X, seed, amp=40.0, base=100.0, noise=4.0).view(frames, slices, Y, X).numpy().astype(np.float32)
