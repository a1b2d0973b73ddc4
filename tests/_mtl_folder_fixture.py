"""tests/golden/ref_model_folder_mtl as the reference wrote it: the checkpoints are committed as `<name>.gz.part<i>` (gzip stream of the
file, cut into pieces below the size limit of a committed file; make_golden_mtl_folder.pack) and are joined and inflated here."""
import gzip
import os
import re
import shutil

TREE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_model_folder_mtl")
_PART = re.compile(r"^(?P<name>.+)\.gz\.part(?P<i>\d+)$")


def unpack(dst):
    """copy the fixture tree to `dst`, every `<name>.gz.part*` group restored to `<name>`; returns dst"""
    for root, _dirs, files in os.walk(TREE):
        out = os.path.join(dst, os.path.relpath(root, TREE))
        os.makedirs(out, exist_ok=True)
        groups = {}
        for fn in files:
            m = _PART.match(fn)
            if m is None:
                shutil.copy(os.path.join(root, fn), os.path.join(out, fn))
            else:
                groups.setdefault(m.group("name"), []).append((int(m.group("i")), fn))
        for name, parts in groups.items():
            z = b"".join(open(os.path.join(root, fn), "rb").read() for _i, fn in sorted(parts))
            with open(os.path.join(out, name), "wb") as f:
                f.write(gzip.decompress(z))
    return dst


def configs():
    """(seg_config, cropping_config): the fixture's YAML values (reduced widths, patch_size [96, 96]) as cineflow.config reads them"""
    from cineflow import config as C
    return tuple(C.read_config(os.path.join(TREE, n), False, False) for n in ("seg_config.yaml", "cropping_config.yaml"))


def mtl_plans(seg_config, crop_config=None, image=96, crop=64, window=8, normalize=False):
    """plans.json of an arch = 'mtl' folder; crop_config=None: no cropping network (the segmenter runs on the whole image)"""
    p = {"num_modalities": 1, "num_classes": 4, "patch_size": [image, image], "image_size": image, "transpose_forward": [0, 1, 2],
         "transpose_backward": [0, 1, 2], "mirror_axes": [0, 1],
         "seg_net": {"arch": "mtl", "config": seg_config, "window_size": window, "normalize": normalize}}
    if crop_config is not None:
        p["crop_size"] = crop
        p["cropping_net"] = {"type": "mtl", "config": crop_config, "window_size": window}
    return p
