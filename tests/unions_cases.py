"""Designs and references shared by tests/test_gpu_unions.py, tests/test_unions_host.py and the child-process
helper tests/unions_nocompact_check.py.

Base design: N = 203 rows in five folds of 67, 33, 41, 40 and 22 rows dealt by a shuffled label vector (fold
position = label), columns with unequal scales (0.5 .. 4) and offsets (-3 .. 3).  Weighted: a tenth of the
weights zero and the whole of fold 4 (22 rows) zero.  Unions: every subset of one to four folds (30).
Oracle references (OracleCVMatrix on the CONCATENATED validation indices) are computed once per
configuration and cached; a union for which the reference raises is recorded with the message."""

import functools
import itertools

import numpy as np

from oracle.cvmatrix_oracle import OracleCVMatrix

N, SIZES = 203, (67, 33, 41, 40, 22)
P = len(SIZES)
SHAPES = ((7, 1), (64, 3), (130, 3), (7, None))          # (K, M); M None: Y absent (training_XTX_unions alone)
FLAGS = ((True, True, True, True), (False, False, False, False), (True, False, True, False),
         (False, True, False, True), (True, True, False, False))       # centre X, centre Y, scale X, scale Y
UNIONS = [list(c) for r in (1, 2, 3, 4) for c in itertools.combinations(range(P), r)]
METHODS = ("XTX", "XTY", "XTX_XTY")


@functools.lru_cache(maxsize=None)
def base_design(K, M, weighted, seed=0):
    """(X, Y | None, w | None, labels, folds): folds[f] = ascending rows of fold f."""
    rng = np.random.default_rng(1000 * K + 10 * (M or 0) + seed)
    X = rng.standard_normal((N, K)) * np.linspace(0.5, 4.0, K) + np.linspace(-3.0, 3.0, K)
    Y = None if M is None else rng.standard_normal((N, M)) * np.linspace(0.5, 4.0, M) + np.linspace(-3.0, 3.0, M)
    labels = rng.permutation(np.repeat(np.arange(P), SIZES)).astype(np.int64)
    w = None
    if weighted:
        w = rng.random(N) + 0.1
        w[rng.choice(N, N // 10, replace=False)] = 0.0
        w[labels == 4] = 0.0
    folds = tuple(np.flatnonzero(labels == f) for f in range(P))
    for a in (X, Y, w, labels) + folds:
        if a is not None:
            a.setflags(write=False)
    return X, Y, w, labels, folds


def union_indices(folds, S):
    return np.concatenate([folds[f] for f in S])


def oracle_call(o, method, val):
    return getattr(o, "training_" + method)(val)


@functools.lru_cache(maxsize=None)
def base_reference(K, M, weighted, flags, method, dtype=np.float64, ddof=1):
    """Per union of UNIONS: the oracle's result ``(mats, stats)``, or the message of its ValueError.  ``dtype``
    float32: the oracle's own float32 arithmetic on the float32-rounded inputs (the yardstick)."""
    X, Y, w, _, folds = base_design(K, M, weighted)
    c = lambda a: None if a is None else a.astype(np.float32).astype(dtype)      # noqa: E731
    o = OracleCVMatrix(*flags, ddof=ddof, dtype=dtype)
    if dtype is np.float32:
        o.fit(c(X), c(Y), c(w))
    else:
        o.fit(X, Y, w)
    out = []
    for S in UNIONS:
        try:
            out.append(oracle_call(o, method, union_indices(folds, S)))
        except ValueError as e:
            out.append(str(e))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rounded_reference(K, M, weighted, flags, method):
    """The float64 oracle on the float32-ROUNDED inputs (what a float32 model is measured against)."""
    X, Y, w, _, folds = base_design(K, M, weighted)
    c = lambda a: None if a is None else a.astype(np.float32).astype(np.float64)      # noqa: E731
    o = OracleCVMatrix(*flags, dtype=np.float64)
    o.fit(c(X), c(Y), c(w))
    out = []
    for S in UNIONS:
        try:
            out.append(oracle_call(o, method, union_indices(folds, S)))
        except ValueError as e:
            out.append(str(e))
    return tuple(out)


def weightless(weighted, S):
    """Does the complement of union S (fold labels) hold no non-zero weight?  (Weighted design: fold 4 is all
    zeros, so the union of folds 0..3.)  With centring or scaling the reference raises for it; without, it
    returns total - update of a matrix whose exact value is ZERO: rounding noise of the size of the operands."""
    return bool(weighted) and sorted(S) == [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def full_scale(K, M, weighted, rounded=False):
    """(max |XTX|, max |XTY|) of the full-data matrices: the operands of the reference's subtraction."""
    X, Y, w, _, _ = base_design(K, M, weighted)
    c = (lambda a: None if a is None else a.astype(np.float32).astype(np.float64)) if rounded else (lambda a: a)   # noqa: E731
    o = OracleCVMatrix(False, False, False, False)
    o.fit(c(X), c(Y), c(w))
    return float(np.abs(o.XTX).max()), (float(np.abs(o.XTY).max()) if Y is not None else 0.0)


def split_result(method, res):
    """(XTX | None, XTY | None, stats) of a method's result."""
    mats, stats = res
    if method == "XTX_XTY":
        return mats[0], mats[1], stats
    return (mats, None, stats) if method == "XTX" else (None, mats, stats)


@functools.lru_cache(maxsize=None)
def split_design(dtype_name, seed=5):
    """N = 1200, K = 130, M = 3, five folds of 240 rows: long enough for forced row-split plans to exist
    (K > 128: an off-diagonal tile, so that a forced plan is taken at all)."""
    n, K, M = 1200, 130, 3
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, K)) * np.linspace(0.5, 4.0, K) + np.linspace(-3.0, 3.0, K)
    Y = rng.standard_normal((n, M)) + 1.0
    w = rng.random(n) + 0.1
    w[rng.choice(n, n // 10, replace=False)] = 0.0
    labels = rng.permutation(np.arange(n) % 5).astype(np.int64)
    dt = np.dtype(dtype_name)
    folds = tuple(np.flatnonzero(labels == f) for f in range(5))
    return X.astype(dt), Y.astype(dt), w.astype(dt), labels, folds


def golden_unions(z):
    uf, uo = z["union_folds"], z["union_offsets"]
    return [list(uf[uo[u]:uo[u + 1]]) for u in range(len(uo) - 1)]


def golden_folds(z):
    """Index arrays of the golden file's folds in the reference Partitioner's order (first appearance)."""
    return [np.flatnonzero(z["labels"] == k) for k in z["fold_keys"]]
