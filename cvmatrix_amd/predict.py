"""Predictions on the device: the out-of-fold predictions of every fold's models (scikit-learn's
``cross_val_predict`` for the whole batch of folds at once) and predictions of one model for new rows.

The fold stage (``CVMatrix.training_XTX_XTY_batched``) and the fitters (``pls_fit_batched``,
``ridge_fit_batched``, ``pcr_fit_batched``) leave an (F, A, K, M) stack of coefficients and the folds'
centring / scaling statistics on the device; ``pls_validation_sse`` reduces the predictions of every
validation row to one sum of squares.  ``cv_predict`` stores the predictions themselves -- for R2 / Q2, MAE,
residuals per row, class decisions of a PLS-DA -- with one launch of ``cvm_cv_predict`` (include/cvmhip.h) and
no wait for the device.  No CPU fallback."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._stage import dtype_code, launch, model_batch, stat_tensors

MAX_RESPONSES = 64
MAX_MODELS = 512


def _check_out(out, shape, dtype, dev):
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise TypeError("out must be a device tensor.")
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {tuple(shape)} {dtype} tensor on {dev} "
                         f"(got {tuple(out.shape)} {out.dtype} on {out.device}).")
    return out


def cv_predict(cvm, folds, stats, B: torch.Tensor, *, order: str = "rows",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Predictions of every fold's models for the fold's own validation rows.

    ``cvm``: a fitted ``CVMatrix`` that keeps device results in float32 or float64 (padded models included;
    Y is not needed); ``folds``: what ``training_XTX_XTY_batched`` was given (a ``Partitioner``, index arrays
    or a ``FoldBatch``); ``stats``: the statistics tuple that call returned, ``(muX, sdX, muY, sdY)`` with
    ``None`` where nothing is centred / scaled (and for the Y side of a model fitted without Y); ``B``: any
    (F, A, K, M) stack of coefficients of this model's dtype on its device.

    ``order="rows"``: returns (N, A, M); ``Yhat[i, a]`` is the prediction for row ``i`` by model ``a`` of the
    fold that holds ``i``.  Rows in no fold are NaN; a row in more than one fold raises ``ValueError``
    (decided on the batch's host indices; a batch made on the device from labels holds every row once).
    ``order="folds"``: returns (n_idx, A, M); row ``p`` belongs to ``batch.idx[p]``, folds may overlap.
    ``out``: a preallocated contiguous tensor of exactly that shape, dtype and device.

    The bits of one prediction depend on its row of X, its fold's statistics and its column of ``B`` alone.
    Runs on the current stream and never waits for the device."""
    if not isinstance(B, torch.Tensor) or not B.is_cuda:
        raise TypeError("cv_predict takes a device tensor of coefficients (F, A, K, M).")
    if order not in ("rows", "folds"):
        raise ValueError("order must be 'rows' or 'folds'.")
    batch, B, (muX, sdX, muY, sdY), max_rows = model_batch("cv_predict", cvm, folds, stats, B)
    F, A, K, M = B.shape
    if not 1 <= M <= MAX_RESPONSES or not 1 <= A <= MAX_MODELS:
        raise ValueError(f"cv_predict takes 1..{MAX_RESPONSES} responses and 1..{MAX_MODELS} models per fold.")
    dev = B.device
    n_idx = int(batch.host_offsets[-1])
    by_row = order == "rows"
    covered = True
    if by_row:
        hidx = batch._host_idx
        if hidx is not None and not batch.is_partition:
            counts = np.bincount(hidx, minlength=cvm.N)
            if counts.size and int(counts.max()) > 1:
                raise ValueError("order='rows': a row is in more than one fold (use order='folds').")
            covered = n_idx == cvm.N
        elif hidx is None:
            covered = n_idx == cvm.N          # (made on the device from labels: every row at most once)
    shape = (cvm.N if by_row else n_idx, A, M)
    lib = _lib.load()
    res = torch.empty(shape, dtype=B.dtype, device=dev) if out is None else _check_out(out, shape, B.dtype, dev)
    if by_row and not covered:
        res.fill_(float("nan"))
    launch("cvm_cv_predict", dev,
           lambda _ws, _n, stream: lib.cvm_cv_predict(
               _lib.ptr(cvm.X), cvm.X.stride(0), _lib.ptr(batch.idx), _lib.ptr(batch.offsets), F, max_rows, K, M, A,
               dtype_code(B.dtype), _lib.ptr(muX), _lib.ptr(sdX), _lib.ptr(muY), _lib.ptr(sdY), _lib.ptr(B),
               _lib.ptr(res), 1 if by_row else 0, stream))
    return res


def predict(X: torch.Tensor, B: torch.Tensor, stats=None) -> torch.Tensor:
    """Predictions of one model for new rows: ``X`` a device tensor (n, K) of ``B``'s dtype with unit column
    stride and any row stride >= K, ``B`` (A, K, M) -- or (K, M), taken as A = 1 -- for instance the refit on
    all rows (the fitters on ``cvm.XTX``, ``cvm.XTY``), ``stats`` None or ``(muX, sdX, muY, sdY)``: 1-D tensors
    of K, K, M, M elements or None.  Returns (n, A, M):
    ``((X - muX) / sdX) @ B[a] * sdY + muY``, with the bits ``cv_predict`` gives the same rows under the same
    model.  Runs on the current stream and never waits for the device."""
    if not (isinstance(X, torch.Tensor) and X.is_cuda and isinstance(B, torch.Tensor) and B.is_cuda):
        raise TypeError("predict takes device tensors X (n, K) and B (A, K, M).")
    if B.dim() == 2:
        B = B.unsqueeze(0)
    if X.dim() != 2 or B.dim() != 3 or X.shape[1] != B.shape[1]:
        raise ValueError("X must be (n, K) and B (A, K, M) or (K, M).")
    if X.dtype != B.dtype or X.device != B.device or X.dtype not in (torch.float64, torch.float32):
        raise ValueError("X and B must both be float64 or both float32, on one device.")
    n, K = X.shape
    A, _, M = B.shape
    if not 1 <= M <= MAX_RESPONSES or not 1 <= A <= MAX_MODELS or K < 1:
        raise ValueError(f"predict takes K >= 1, 1..{MAX_RESPONSES} responses and 1..{MAX_MODELS} models.")
    if (K > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < K):
        raise ValueError("X must have unit column stride and a row stride >= K.")
    dev = X.device
    muX, sdX, muY, sdY = stat_tensors((None,) * 4 if stats is None else stats, None, K, M, B.dtype, dev)
    B = B.contiguous()
    lib = _lib.load()
    res = torch.empty((n, A, M), dtype=B.dtype, device=dev)
    if n == 0:
        return res
    offsets = torch.arange(0, n + 1, n, dtype=torch.int64, device=dev)      # {0, n}, made on the device: no copy to wait for
    launch("cvm_cv_predict", dev,
           lambda _ws, _n, stream: lib.cvm_cv_predict(
               _lib.ptr(X), max(X.stride(0), K), 0, _lib.ptr(offsets), 1, n, K, M, A, dtype_code(B.dtype),
               _lib.ptr(muX), _lib.ptr(sdX), _lib.ptr(muY), _lib.ptr(sdY), _lib.ptr(B), _lib.ptr(res), 0, stream))
    return res
