#!/usr/bin/env python3
"""Generate tests/golden/validate/splits.json: the five-fold split the fork's do_split makes for 10 and for 12 cases.

    python tests/golden/make_golden_validate.py

The folds come from scikit-learn itself -- KFold(n_splits=5, shuffle=True, random_state=12345) over the PAIRS of adjacent sorted case
names, each pair index i standing for the cases 2 i and 2 i + 1 (nnUNetTrainerV2.py:299-319) -- so that cineflow.validate.do_split, which
restates KFold's seeded shuffle-and-cut in numpy, is checked against the library where it is installed and against this file where it
is not.  Only names and lists are stored."""
import json
import os

import numpy as np
from sklearn.model_selection import KFold

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "validate")


def case_names(n):
    # two frames per patient, as the cine tasks name them; deliberately generated out of order
    names = ["patient%03d_frame%02d" % (p, f) for p in range(n // 2) for f in (9, 1)]
    return names[::-1]


def fork_splits(keys):
    keys = np.sort(list(keys))
    pairs = np.arange(len(keys) // 2)
    splits = []
    for train_pairs, test_pairs in KFold(n_splits=5, shuffle=True, random_state=12345).split(pairs):
        train = np.sort(np.concatenate([train_pairs * 2, train_pairs * 2 + 1]))
        test = np.sort(np.concatenate([test_pairs * 2, test_pairs * 2 + 1]))
        assert len(train) + len(test) == len(keys)
        splits.append({"train": [str(k) for k in keys[train]], "val": [str(k) for k in keys[test]]})
    return splits


def main():
    os.makedirs(OUT, exist_ok=True)
    doc = {}
    for n in (10, 12):
        keys = case_names(n)
        doc[str(n)] = {"keys": keys, "splits": fork_splits(keys)}
    with open(os.path.join(OUT, "splits.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(OUT, "splits.json"))


if __name__ == "__main__":
    main()
