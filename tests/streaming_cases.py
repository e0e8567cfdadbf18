"""Chunkings and references shared by tests/test_streaming_host.py and tests/test_gpu_streaming.py.

Designs come from tests/unions_cases.py (base design: 203 rows, five shuffled folds; weighted: a tenth of the
weights zero and fold 4 all zero).  Chunkings of its rows:
  A  one chunk
  B  rows [0:80] [80:81] [81:203] with an empty chunk in between: a one-row chunk, folds missing from a chunk,
     a no-op
  C  rows sorted by label, one fold per chunk: every chunk misses four folds
  D  chunking B fed in reverse order
Reference: OracleCVMatrix fitted on ALL rows, each fold's rows as validation indices -- computed once per
configuration and cached; a fold for which the reference raises is recorded with the message."""

import functools

import numpy as np

import unions_cases as uc
from oracle.cvmatrix_oracle import OracleCVMatrix

CHUNKINGS = ("A", "B", "C", "D")


def chunk_rows(name, labels):
    """The row-index arrays of chunking ``name``, in feeding order."""
    n = len(labels)
    if name == "A":
        return [np.arange(n)]
    if name in ("B", "D"):
        rows = [np.arange(0, 80), np.arange(0), np.arange(80, 81), np.arange(81, n)]
        return rows if name == "B" else rows[::-1]
    if name == "C":
        return [np.flatnonzero(labels == f) for f in range(int(labels.max()) + 1)]
    raise KeyError(name)


def feed(scv, X, Y, w, labels, rows, conv=lambda a: a):
    """``partial_fit`` of every chunk; ``conv`` turns a chunk's array into what is handed over."""
    for r in rows:
        scv.partial_fit(conv(X[r]), None if Y is None else conv(Y[r]), None if w is None else conv(w[r]), labels[r])
    return scv


def _per_fold(o, folds, call):
    out = []
    for v in folds:
        try:
            out.append(call(o, v))
        except ValueError as e:
            out.append(str(e))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fold_reference(K, M, weighted, flags, method, ddof=1):
    """Per fold of the base design: the float64 oracle's ``training_<method>`` result, or its message."""
    X, Y, w, _, folds = uc.base_design(K, M, weighted)
    o = OracleCVMatrix(*flags, ddof=ddof, dtype=np.float64)
    o.fit(X, Y, w)
    return _per_fold(o, folds, lambda o_, v: uc.oracle_call(o_, method, v))


@functools.lru_cache(maxsize=None)
def statistics_reference(K, M, weighted, flags):
    X, Y, w, _, folds = uc.base_design(K, M, weighted)
    o = OracleCVMatrix(*flags, dtype=np.float64)
    o.fit(X, Y, w)
    return _per_fold(o, folds, lambda o_, v: o_.training_statistics(v))


@functools.lru_cache(maxsize=None)
def attribute_reference(K, M, weighted, flags):
    """The oracle's full-data attributes (None where the flags do not ask for one)."""
    X, Y, w, _, _ = uc.base_design(K, M, weighted)
    o = OracleCVMatrix(*flags, dtype=np.float64)
    o.fit(X, Y, w)
    return {n: getattr(o, n) for n in ("XTX", "XTY", "sum_X", "sum_sq_X", "sum_Y", "sum_sq_Y", "sum_w", "num_nonzero_w")}


@functools.lru_cache(maxsize=None)
def fold_reference32(K, M, weighted, flags):
    """(float64 oracle on the float32-ROUNDED inputs, the float32 oracle on them: the yardstick), per fold,
    method XTX_XTY."""
    X, Y, w, _, folds = uc.base_design(K, M, weighted)
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: None if a is None else a.astype(np.float32).astype(dt)      # noqa: E731
        o = OracleCVMatrix(*flags, dtype=dt)
        o.fit(c(X), c(Y), c(w))
        out.append(_per_fold(o, folds, lambda o_, v: o_.training_XTX_XTY(v)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def split_reference(dtype_name, flags):
    """uc.split_design (1200 rows, K = 130): (float64 oracle on the design's own -- already rounded -- values,
    the oracle in the design's dtype), per fold, method XTX_XTY."""
    X, Y, w, _, folds = uc.split_design(dtype_name)
    out = []
    for dt in (np.float64, np.dtype(dtype_name).type):
        o = OracleCVMatrix(*flags, dtype=dt)
        o.fit(X.astype(dt), Y.astype(dt), w.astype(dt))
        out.append(_per_fold(o, folds, lambda o_, v: o_.training_XTX_XTY(v)))
    return tuple(out)


def fp32_errors(got, r64, r32):
    """(error of ``got``, the yardstick: error of the float32 oracle), both against the float64 oracle on the
    rounded inputs, norm-wise in the scale of that reference."""
    r64 = np.asarray(r64, dtype=np.float64)
    scale = np.abs(r64).max()
    return (float(np.abs(np.asarray(got, dtype=np.float64) - r64).max() / scale),
            float(np.abs(np.asarray(r32, dtype=np.float64) - r64).max() / scale))
