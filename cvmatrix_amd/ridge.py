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
    lam = np.asarray(lambdas, dtype=np.float64)
    if lam.ndim != 1:
        raise ValueError(f"lambdas must be one-dimensional, got shape {lam.shape}.")
    if not 1 <= lam.size <= MAX_PENALTIES:
        raise ValueError(f"lambdas must hold 1 to {MAX_PENALTIES} values, got {lam.size}.")
    if not np.all(np.isfinite(lam)) or np.any(lam < 0):
        raise ValueError("every lambda must be finite and >= 0.")
    return np.ascontiguousarray(lam)


def ridge_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, lambdas, *, check: bool = False) -> RidgeFit:
    """Ridge coefficients for every fold and every penalty: ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device
    tensors (the outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is taken as
    F = 1), ``lambdas`` anything ``np.asarray`` turns into a 1-D float64 array.

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``info`` once and
    raises ``numpy.linalg.LinAlgError`` naming the first (fold, lambda, pivot) whose matrix was not
    positive definite."""
    if not (isinstance(XTX, torch.Tensor) and XTX.is_cuda and isinstance(XTY, torch.Tensor) and XTY.is_cuda):
        raise TypeError("ridge_fit_batched takes device tensors (the batched training matrices).")
    if XTX.dim() == 2:
        XTX = XTX.unsqueeze(0)
        XTY = XTY.unsqueeze(0) if XTY.dim() == 2 else XTY.reshape(1, -1, 1)
    if XTX.dim() != 3 or XTY.dim() != 3 or XTX.shape[1] != XTX.shape[2] or XTY.shape[:2] != XTX.shape[:2]:
        raise ValueError("XTX must be (F,K,K) and XTY (F,K,M).")
    if XTX.dtype != XTY.dtype or XTX.dtype not in (torch.float64, torch.float32):
        raise ValueError("XTX and XTY must both be float64 or both float32.")
    if XTX.device != XTY.device:
        raise ValueError("XTX and XTY must be on one device.")
    F, K, M = XTY.shape
    if not 1 <= K <= MAX_K:
        raise ValueError(f"The device ridge takes 1 <= K <= {MAX_K}.")
    if not 1 <= M <= MAX_RESPONSES:
        raise ValueError(f"The device ridge takes 1 to {MAX_RESPONSES} responses.")
    lam = check_lambdas(lambdas)
    L = lam.size
    XTX = XTX.contiguous()
    XTY = XTY.contiguous()
    lib = _lib.load()
    dev = XTX.device
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    with torch.cuda.device(dev):
        one = lib.cvm_ridge_workspace_bytes(1, K, M, 1)
        nbytes = min(lib.cvm_ridge_workspace_bytes(F, K, M, L), max(one, WORKSPACE_LIMIT))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        B = torch.empty((F, L, K, M), dtype=XTX.dtype, device=dev)
        info = torch.empty((F, L), dtype=torch.int32, device=dev)
        if F == 0:                # nothing to launch (and empty tensors have no address to hand over)
            return RidgeFit(B, info)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.cvm_ridge_fit(_lib.ptr(XTX), _lib.ptr(XTY), F, K, M, lam.ctypes.data, L, code, _lib.ptr(B),
                               _lib.ptr(info), _lib.ptr(ws), nbytes, stream)
        _lib.check(rc, "cvm_ridge_fit")
        ws.record_stream(torch.cuda.current_stream(dev))
        if check and F:
            host = info.cpu().numpy()
            bad = np.argwhere(host != 0)
            if bad.size:
                f, l = (int(v) for v in bad[0])
                raise np.linalg.LinAlgError(
                    f"ridge_fit_batched: fold {f}, lambda[{l}] = {lam[l]!r}: pivot {int(host[f, l])} is not "
                    f"positive (XTX + lambda I is not positive definite); {len(bad)} problem(s) failed.")
    return RidgeFit(B, info)
