"""Ridge regression over a grid of penalties on the training matrices of a batch of folds, on the
device: ``B(lambda) = (XTX + lambda I)^-1 XTY`` for every fold and every lambda, by one launch of
``cvm_ridge_fit`` (include/cvmhip.h) -- a Cholesky factorisation per (fold, lambda) in float64.

The coefficients have the layout ``pls_validation_sse`` scores, with lambda in place of the number of
components: ``pls_validation_sse(cvm, folds, stats, fit.B)`` and ``cv_rmse`` give the cross-validated
RMSE per lambda.  No CPU fallback."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._stage import check_fit_dims, check_grid, dtype_code, launch, training_pair

MAX_K = 4096
MAX_RESPONSES = 64
MAX_PENALTIES = 256
WORKSPACE_LIMIT = 4 << 30     # bytes; fewer problems run at once beyond it (same results to the bit)


class RidgeFit(NamedTuple):
    """``B`` (F, L, K, M) in the dtype of XTX: ``B[f, l]`` = coefficients of fold f with penalty
    ``lambdas[l]``; ``info`` (F, L) int32 on the device: 0, or j > 0 where pivot j (1-based) was not
    positive -- ``B[f, l]`` is then NaN.  A NaN in ``XTY`` alone is no failure: ``info`` stays 0,
    the columns of ``B[f, l]`` whose right-hand side held it are NaN, the other columns are unaffected."""
    B: torch.Tensor
    info: torch.Tensor


def check_lambdas(lambdas) -> np.ndarray:
    """The penalty grid as a contiguous 1-D float64 array: 1 to 256 values, each finite and >= 0."""
    return check_grid("lambdas", lambdas, MAX_PENALTIES, low_open=False)


def ridge_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, lambdas, *, check: bool = False) -> RidgeFit:
    """Ridge coefficients for every fold and every penalty: ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device
    tensors (the outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is taken as
    F = 1), ``lambdas`` anything ``np.asarray`` turns into a 1-D float64 array.

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``info`` once and
    raises ``numpy.linalg.LinAlgError`` naming the first (fold, lambda, pivot) whose matrix was not
    positive definite."""
    XTX, XTY, F, K, M = training_pair("ridge_fit_batched", XTX, XTY)
    check_fit_dims("The device ridge", K, M, MAX_K, MAX_RESPONSES)
    lam = check_lambdas(lambdas)
    L = lam.size
    dev = XTX.device
    B = torch.empty((F, L, K, M), dtype=XTX.dtype, device=dev)
    info = torch.empty((F, L), dtype=torch.int32, device=dev)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return RidgeFit(B, info)
    lib = _lib.load()
    launch("cvm_ridge_fit", dev,
           lambda ws, nbytes, stream: lib.cvm_ridge_fit(
               _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, lam.ctypes.data, L, dtype_code(XTX.dtype), _lib.ptr(B),
               _lib.ptr(info), ws, nbytes, stream),
           lib.cvm_ridge_workspace_bytes(F, K, M, L), one=lib.cvm_ridge_workspace_bytes(1, K, M, 1),
           limit=WORKSPACE_LIMIT)
    if check:
        host = info.cpu().numpy()
        bad = np.argwhere(host != 0)
        if bad.size:
            f, l = (int(v) for v in bad[0])
            raise np.linalg.LinAlgError(
                f"ridge_fit_batched: fold {f}, lambda[{l}] = {lam[l]!r}: pivot {int(host[f, l])} is not "
                f"positive (XTX + lambda I is not positive definite); {len(bad)} problem(s) failed.")
    return RidgeFit(B, info)
