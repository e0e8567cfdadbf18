"""Unions of folds for nested (double) cross-validation and repeated leave-several-groups-out.

``CVMatrix.training_XTX_XTY_unions(folds, unions)`` returns the training matrices of "all rows except the
folds of union u" for every union, formed on the device from the partials one sweep left behind
(``cvm_sweep_unions``: ``G - sum_{f in S} U_f``, no row of X read again).  This module holds the host side:
the lists of unions nested cross-validation needs, and the check / CSR form of a caller's list.

Nested cross-validation over P folds: for every outer fold f the inner loop trains without f AND one inner
fold g != f and scores on g -- the training matrices are those of the pair {f, g}, the same for (f, g) and
(g, f); ``fold_pairs`` lists the pairs once, ``nested_units`` says which pair and which validation fold
each (outer, inner) unit uses."""

from __future__ import annotations

import numpy as np

__all__ = ["fold_pairs", "nested_units", "UnionBatch", "prepare_unions"]


def fold_pairs(P: int) -> np.ndarray:
    """Every pair of folds ``(f, g)`` with ``f < g`` of ``P`` folds: int64 ``(P (P - 1) / 2, 2)``, row-major
    in f -- (0,1), (0,2) .. (0,P-1), (1,2) .."""
    P = int(P)
    if P < 0:
        raise ValueError("P must be >= 0")
    f, g = np.triu_indices(P, k=1)
    return np.stack([f, g], axis=1).astype(np.int64)


def _pair_index(f, g, P: int):
    """Row of the pair {f, g} in ``fold_pairs(P)``."""
    lo, hi = np.minimum(f, g), np.maximum(f, g)
    return lo * P - lo * (lo + 1) // 2 + (hi - lo - 1)


def nested_units(P: int):
    """Every ordered (outer f, inner g != f) of ``P`` folds, outer-major, inner ascending, as three int64
    arrays of length ``P (P - 1)``: ``outer``, ``pair`` (the row of {f, g} in ``fold_pairs(P)``: the model of
    the unit is trained without f and g) and ``inner`` (= g: the fold the unit's model is scored on)."""
    P = int(P)
    if P < 0:
        raise ValueError("P must be >= 0")
    outer, inner = np.nonzero(~np.eye(P, dtype=bool))
    outer, inner = outer.astype(np.int64), inner.astype(np.int64)
    return outer, _pair_index(outer, inner, P).astype(np.int64), inner


class UnionBatch:
    """A checked list of unions in CSR form: ``folds`` (int64, every union's fold positions ascending),
    ``offsets`` (int64 ``[n + 1]``); uploaded once per device on first use."""

    def __init__(self, folds: np.ndarray, offsets: np.ndarray, n_folds: int) -> None:
        self.folds, self.offsets, self.n_folds = folds, offsets, int(n_folds)
        self._dev = {}

    @property
    def n_unions(self) -> int:
        return len(self.offsets) - 1

    def device(self, device):
        """(folds, offsets) as tensors on ``device``."""
        import torch

        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = (torch.from_numpy(self.folds).to(device), torch.from_numpy(self.offsets).to(device))
        return t


def prepare_unions(unions, n_folds: int) -> UnionBatch:
    """Check ``unions`` -- a sequence of sequences of fold positions, or an ``(n, r)`` integer array --
    against ``n_folds`` folds and put it in CSR form, every union's positions ascending (the order inside
    a union does not matter).  ``ValueError`` for an empty union, a repeated fold, a position out of range."""
    if isinstance(unions, UnionBatch):
        if unions.n_folds != n_folds:
            raise ValueError(f"these unions were prepared for {unions.n_folds} folds, the batch has {n_folds}")
        return unions
    if hasattr(unions, "detach"):
        unions = unions.detach().cpu().numpy()
    if isinstance(unions, np.ndarray):
        if unions.ndim != 2:
            raise ValueError("unions as an array must have shape (n, r): one row of fold positions per union")
        rows = list(unions)
    else:
        rows = list(unions)
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    parts = []
    for u, row in enumerate(rows):
        r = np.asarray(row)
        if r.ndim != 1:
            raise ValueError(f"union {u}: expected a sequence of fold positions")
        if r.size == 0:
            raise ValueError(f"union {u} is empty")
        if r.dtype.kind not in "iu":
            raise ValueError(f"union {u}: fold positions must be integers")
        r = np.sort(r.astype(np.int64))
        if r[0] < 0 or r[-1] >= n_folds:
            raise ValueError(f"union {u}: fold position out of range for {n_folds} folds")
        if r.size > 1 and bool(np.any(r[1:] == r[:-1])):
            raise ValueError(f"union {u} repeats a fold")
        parts.append(r)
        offsets[u + 1] = offsets[u] + r.size
    folds = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return UnionBatch(np.ascontiguousarray(folds, dtype=np.int64), offsets, n_folds)
