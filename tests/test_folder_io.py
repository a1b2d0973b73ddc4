"""cineflow.folder_io without a GPU: the read-ahead generator (order, depth bound, where a reader's exception surfaces, the life of its pool),
the geometry check of a saved softmax case, and the old import paths of the names that moved there."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

WAIT = 5.0                                                         # only ever waited out by a failing test


def test_read_ahead_yields_every_group_in_order():
    from cineflow.folder_io import read_ahead
    groups = [(1, 2, 3), (), (4,), (5, 6), (), ()]
    for depth in (1, 2, 3, 10):
        got = list(read_ahead(groups, lambda x: x * x, depth=depth))
        assert got == [(g, [x * x for x in g]) for g in groups], depth
    assert list(read_ahead([], lambda x: x)) == []
    assert list(read_ahead(iter([(7,)]), str)) == [((7,), ["7"])]  # any iterable of groups


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_read_ahead_starts_no_more_than_depth_groups_beyond_the_current_one(depth):
    from cineflow.folder_io import read_ahead
    n = 7
    started, lock = set(), threading.Lock()
    release = [threading.Event() for _ in range(n)]

    def read(g):
        with lock:
            started.add(g)
        assert release[g].wait(WAIT)
        return g

    release[0].set()
    gen = read_ahead([(g, g) for g in range(n)], read, depth=depth, readers=2 * n)
    for i, (group, loaded) in enumerate(gen):
        assert group == (i, i) and loaded == [i, i]
        with lock:
            assert max(started) <= i + depth, (i, sorted(started))
        if i + 1 < n:
            release[i + 1].set()
    assert started == set(range(n))


def test_a_readers_exception_surfaces_at_its_group():
    from cineflow.folder_io import read_ahead

    def read(x):
        if x == 20:
            raise KeyError("group 2")
        return x
    gen = read_ahead([(0,), (10, 11), (20, 21), (30,)], read, depth=3)
    assert next(gen) == ((0,), [0])
    assert next(gen) == ((10, 11), [10, 11])
    with pytest.raises(KeyError, match="group 2"):
        next(gen)
    with pytest.raises(StopIteration):
        next(gen)


@pytest.fixture
def made_pools(monkeypatch):
    """the executors that folder_io creates while the test runs"""
    from cineflow import folder_io
    made = []

    def factory(*a, **k):
        made.append(ThreadPoolExecutor(*a, **k))
        return made[-1]
    monkeypatch.setattr(folder_io, "ThreadPoolExecutor", factory)
    return made


def _is_shut_down(pool):
    with pytest.raises(RuntimeError):
        pool.submit(int)
    return True


def test_a_pool_of_its_own_is_shut_down_however_the_generator_ends(made_pools):
    from cineflow.folder_io import read_ahead
    groups = [(i,) for i in range(5)]
    assert len(list(read_ahead(groups, int, depth=2, readers=3))) == 5             # exhausted
    assert len(made_pools) == 1 and made_pools[0]._max_workers == 3 and _is_shut_down(made_pools[0])

    gen = read_ahead(groups, int, depth=2)
    next(gen)
    gen.close()                                                                    # the consumer stops early
    assert len(made_pools) == 2 and made_pools[1]._max_workers == 2 and _is_shut_down(made_pools[1])

    def read(x):
        raise OSError("unreadable")
    with pytest.raises(OSError, match="unreadable"):
        list(read_ahead(groups, read))
    assert len(made_pools) == 3 and _is_shut_down(made_pools[2])


def test_the_callers_pool_is_used_and_left_running(made_pools):
    from cineflow.folder_io import read_ahead
    names = set()

    def read(x):
        names.add(threading.current_thread().name)
        return x
    with ThreadPoolExecutor(2, thread_name_prefix="callers") as pool:
        gen = read_ahead([(1,), (2,), (3,)], read, pool=pool)
        next(gen)
        gen.close()
        assert pool.submit(int, "4").result() == 4
        assert len(list(read_ahead([(1,), (2,)], read, pool=pool))) == 2
        assert pool.submit(int, "5").result() == 5
    assert made_pools == [] and names and all(n.startswith("callers") for n in names)


def _props(after, full=None, lo=None):
    p = {"size_after_cropping": tuple(after)}
    if full is not None:
        p["original_size_of_raw_data"] = np.array(full)
        p["crop_bbox"] = [[a, a + n] for a, n in zip(lo, after)]
    return p


def test_softmax_case_geometry_results_and_refusals():
    from cineflow.folder_io import softmax_case_geometry as geometry
    assert geometry((2, 1, 2, 3), _props((1, 2, 3), (1, 2, 3), (0, 0, 0)), "c") == ((1, 2, 3), (0, 0, 0))
    assert geometry((2, 1, 2, 3), _props((1, 2, 3)), "c") == ((1, 2, 3), (0, 0, 0))                       # no crop_bbox: the crop is the volume
    assert geometry((4, 3, 5, 7), _props((3, 5, 7), (4, 9, 8), (1, 4, 1)), "c") == ((4, 9, 8), (1, 4, 1))   # lo + crop == full on every axis
    assert geometry(np.zeros((2, 1, 2, 3), np.float16).shape, _props(np.array([1, 2, 3]), (5, 6, 7), (2, 0, 1)), "c") == ((5, 6, 7), (2, 0, 1))
    with pytest.raises(ValueError, match=r"a/c2\.npz.*\(1, 2, 3\).*size_after_cropping is \(1, 4, 6\)"):
        geometry((2, 1, 2, 3), _props((1, 4, 6), (1, 4, 6), (0, 0, 0)), "a/c2.npz")
    with pytest.raises(ValueError, match=r"a/c3\.npz.*\(1, 2, 3\) at \(0, 0, 2\) overhangs original_size_of_raw_data \(1, 2, 4\)"):
        geometry((2, 1, 2, 3), _props((1, 2, 3), (1, 2, 4), (0, 0, 2)), "a/c3.npz")
    with pytest.raises(ValueError, match="overhangs"):
        geometry((2, 1, 2, 3), _props((1, 2, 3), (1, 2, 4), (0, -1, 0)), "c")                             # a negative origin
    with pytest.raises(ValueError, match="overhangs"):
        geometry((2, 1, 2, 3), _props((1, 2, 3), (2, 4), (0, 0, 0)), "c")                                 # a volume that is not 3-D
    with pytest.raises(ValueError, match="size_after_cropping"):
        geometry((1, 2, 3), _props((2, 3)), "c")                                                          # a softmax that is not [K,Z,Y,X]


def test_load_softmax_reads_the_softmax_entry(tmp_path):
    from cineflow.folder_io import load_softmax
    sm = np.arange(24, dtype=np.float16).reshape(2, 1, 3, 4)
    np.savez_compressed(str(tmp_path / "c.npz"), softmax=sm)
    got = load_softmax(str(tmp_path / "c.npz"))
    assert got.dtype == sm.dtype and np.array_equal(got, sm)


def test_the_old_import_paths_name_the_same_objects():
    from cineflow import evaluation, export, folder_io, metrics, postprocessing, score
    assert export.subfiles is folder_io.subfiles
    assert evaluation.save_json is folder_io.save_json and score.save_json is folder_io.save_json
    assert evaluation.load_volume is folder_io.load_volume and evaluation.Loaded is folder_io.Loaded
    assert postprocessing.load_json is folder_io.load_json
    assert evaluation.label_volume_u8 is metrics.label_volume_u8
