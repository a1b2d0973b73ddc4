"""What the folder tools share on the host: listing a folder, JSON in and out, reading a label file, reading cases ahead of the device,
and the geometry check of a saved softmax case.  Nothing here touches the device: the module imports neither torch nor the library."""
import collections
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .nifti import read_nifti

join = os.path.join

# a volume that is already in memory: (file name it stands for, array [Z,Y,X], read_nifti's properties)
Loaded = collections.namedtuple("Loaded", "path array props")


def subfiles(folder, suffix=None, join_=True, sort=True):
    res = [f for f in os.listdir(folder) if os.path.isfile(join(folder, f)) and (suffix is None or f.endswith(suffix))]
    if sort:
        res.sort()
    return [join(folder, f) for f in res] if join_ else res


def load_json(file):
    with open(file) as f:
        return json.load(f)


def save_json(obj, file, indent=4, sort_keys=True):
    with open(file, "w") as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


def load_volume(path):
    array, props = read_nifti(path)
    return Loaded(path, array, props)


def read_ahead(groups, read, depth=1, pool=None, readers=None):
    """Generator of (group, [read(item) for item in group]) in the order of `groups`, the reads done by a thread pool while the caller works:
    when a group is yielded, the next `depth` (>= 1) groups are submitted and no later one.  A reader's exception is raised where its group
    would have been yielded.  pool: the caller's executor, left running; without one a pool of `readers` threads (default: depth) is made
    and shut down when the generator ends, however it ends."""
    groups, depth = list(groups), max(1, int(depth))
    own = pool is None
    pool = ThreadPoolExecutor(max(1, int(readers or depth))) if own else pool
    try:
        ahead = collections.deque([pool.submit(read, item) for item in g] for g in groups[:depth])
        for i, group in enumerate(groups):
            loaded = [f.result() for f in ahead.popleft()]
            if i + depth < len(groups):
                ahead.append([pool.submit(read, item) for item in groups[i + depth]])
            yield group, loaded
    finally:
        if own:
            pool.shutdown(wait=True, cancel_futures=True)


def load_softmax(path):
    return np.load(path, allow_pickle=False)["softmax"]


def softmax_case_geometry(shape, props, what):
    """shape [K,Z,Y,X] of a case's saved softmax and its properties -> (full, lo): the size of the label volume before cropping and the crop's
    origin in it.  Refused when the softmax is not of the properties' size_after_cropping or the crop overhangs the volume."""
    crop = tuple(int(v) for v in shape[1:])
    after = tuple(int(v) for v in props["size_after_cropping"])
    if len(shape) != 4 or crop != after:
        raise ValueError("%s: softmax of size %s, size_after_cropping is %s (nothing is resampled here)" % (what, crop, after))
    bbox = props.get("crop_bbox")
    if bbox is None:
        return crop, (0, 0, 0)
    full = tuple(int(v) for v in props["original_size_of_raw_data"])
    lo = tuple(int(b[0]) for b in bbox)
    if len(full) != 3 or any(a < 0 or a + n > f for a, n, f in zip(lo, crop, full)):
        raise ValueError("%s: the crop %s at %s overhangs original_size_of_raw_data %s" % (what, crop, lo, full))
    return full, lo
