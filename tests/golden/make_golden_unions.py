"""
Generate tests/golden/g9_unions.npz by IMPORTING THE REFERENCE (sm00thix/cvmatrix): the training matrices of
the complements of unions of folds, i.e. the reference's ``training_XTX_XTY`` on the CONCATENATED validation
indices of the folds of every union.  Run where the reference is checked out (it is not part of this
repository), with its location as the argument:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unions.py <path to the reference checkout>

The file holds arrays only: the inputs (N = 60, K = 5, M = 2, weighted, five folds by a shuffled label
vector), the unions (all ten pairs and one triple, CSR) and, for the flag sets 1111 and 0000, the
reference's XTX, XTY and statistics of every union.
"""

import itertools
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
STAT_NAMES = ("muX", "sdX", "muY", "sdY")
N, K, M, P = 60, 5, 2, 5
UNIONS = [list(c) for c in itertools.combinations(range(P), 2)] + [[0, 2, 4]]


def inputs():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((N, K)) * np.linspace(0.5, 4.0, K) + np.linspace(-3.0, 3.0, K)
    Y = rng.standard_normal((N, M)) * np.array([1.0, 2.5]) + np.array([0.5, -2.0])
    w = rng.random(N) + 0.1
    w[rng.choice(N, N // 10, replace=False)] = 0.0
    labels = rng.permutation(np.arange(N) % P)
    return X, Y, w, labels


def main():
    sys.path.insert(0, sys.argv[1])
    from cvmatrix import CVMatrix, Partitioner

    X, Y, w, labels = inputs()
    p = Partitioner(labels)
    keys = list(p.folds_dict)
    out = {"X": X, "Y": Y, "w": w, "labels": labels.astype(np.int64),
           "fold_keys": np.asarray(keys, dtype=np.int64),
           "union_folds": np.concatenate([np.asarray(u, dtype=np.int64) for u in UNIONS]),
           "union_offsets": np.cumsum([0] + [len(u) for u in UNIONS]).astype(np.int64)}
    for name, flags in (("1111", (True,) * 4), ("0000", (False,) * 4)):
        m = CVMatrix(*flags, 1, np.float64, True, backend="numpy")
        m.fit(X, Y, w)
        for u, S in enumerate(UNIONS):
            val = np.concatenate([p.get_validation_indices(keys[f]) for f in S])
            (xtx, xty), stats = m.training_XTX_XTY(val)
            out[f"{name}/{u}/XTX"], out[f"{name}/{u}/XTY"] = np.asarray(xtx), np.asarray(xty)
            mask = np.zeros(4, dtype=bool)
            for i, (n, s) in enumerate(zip(STAT_NAMES, stats)):
                if s is not None:
                    mask[i] = True
                    out[f"{name}/{u}/{n}"] = np.asarray(s)
            out[f"{name}/{u}/mask"] = mask
    np.savez_compressed(os.path.join(HERE, "g9_unions.npz"), **out)
    print("wrote g9_unions.npz:", len(UNIONS), "unions")


if __name__ == "__main__":
    main()
