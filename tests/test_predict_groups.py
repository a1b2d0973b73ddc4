"""CPU tests (no device) of cineflow.predict._groups, the rule that fills the device batches of the file-level API: a patient joins the
group unless the group is non-empty and would exceed the cap; the cap starts at min(max_slices, first) and doubles up to max_slices after
every group.  The expected groups were obtained by simulating the loop that `_predict_patients` held before the rule became a generator."""
import pytest


def _pairs(slices):
    return list(enumerate(slices))


@pytest.mark.parametrize("slices, max_slices, first, expected", [
    ([2, 3, 2], 5, 16, [[0, 1], [2]]),
    ([2, 3, 2], 1, 16, [[0], [1], [2]]),                    # a patient larger than the cap goes alone, never dropped
    ([4] * 7, 16, 4, [[0], [1, 2], [3, 4, 5, 6]]),          # caps 4, 8, 16
    ([3, 9, 2], 5, 16, [[0], [1], [2]]),
])
def test_groups_follow_the_greedy_rule_and_the_doubling_cap(slices, max_slices, first, expected):
    from cineflow.predict import _groups
    assert list(_groups(iter(_pairs(slices)), max_slices, first)) == expected


def test_groups_of_the_api_benchmark_shape():
    """16 patients of 8 slices, caps 16, 32, 64, 64 (bench.py --variant api): four device batches"""
    from cineflow.predict import _groups
    groups = list(_groups(iter(_pairs([8] * 16)), 64, 16))
    assert [len(g) for g in groups] == [2, 4, 8, 2]
    assert [i for g in groups for i in g] == list(range(16))


def test_groups_pull_one_item_past_the_group_and_no_further():
    """the overlap of preprocessing with the device depends on it: when a group comes out, exactly one item beyond it has been taken from
    the iterator (the first of the next group), and at the end every item has been taken exactly once"""
    from cineflow.predict import _groups
    pulled = []

    def recording():
        for pair in _pairs([4] * 7):
            pulled.append(pair[0])
            yield pair

    gen = _groups(recording(), 16, 4)
    assert next(gen) == [0] and pulled == [0, 1]
    assert next(gen) == [1, 2] and pulled == [0, 1, 2, 3]
    assert next(gen) == [3, 4, 5, 6] and pulled == list(range(7))
    with pytest.raises(StopIteration):
        next(gen)
    assert pulled == list(range(7))


def test_groups_of_nothing():
    from cineflow.predict import _groups
    assert list(_groups(iter(()), 64, 16)) == []
