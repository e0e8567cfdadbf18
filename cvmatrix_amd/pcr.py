"""PCA and principal component regression on the training matrices of a batch of folds, on the device:
the leading eigenpairs of every ``XTX[f]`` and the coefficients ``B[f, a] = sum_{j<=a} v_j (v_j^T XTY[f]) /
lambda_j`` with 1 .. A components, by one launch of ``cvm_pcr_fit`` (include/cvmhip.h) -- a cyclic Jacobi
eigensolver per fold in float64.

The coefficients have the layout ``pls_validation_sse`` scores: ``pls_validation_sse(cvm, folds, stats,
fit.B)`` and ``cv_rmse`` give the cross-validated RMSE per number of components.  No CPU fallback."""

from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

MAX_K = 512
MAX_RESPONSES = 64
MAX_SWEEPS = 60
WORKSPACE_LIMIT = 4 << 30     # bytes; fewer folds run at once beyond it (same results to the bit)


class PCRFit(NamedTuple):
    """``B`` (F, A, K, M) in the dtype of XTX: ``B[f, a]`` = coefficients of fold f on its first a+1
    principal components -- the layout ``pls_validation_sse`` scores; None for PCA only.  ``eigenvalues``
    (F, A) float64, descending.  ``components`` (F, K, A) in the dtype of XTX (None unless asked for): unit
    vectors whose entry of largest magnitude is positive; components that do not exist are zero.  ``n_fit``
    (F,) int32: the components that exist (eigenvalue above ``rank_tol`` times the largest), at most A;
    ``B[f, a]`` for ``a >= n_fit[f]`` repeats ``B[f, n_fit[f] - 1]``.  ``sweeps`` (F,) int32: Jacobi sweeps run.
    A fold with a NaN or an infinity in its matrices is NaN throughout with ``n_fit`` -1 and ``sweeps`` 0; a
    fold that did not converge in 60 sweeps likewise with ``sweeps`` -1."""
    B: Optional[torch.Tensor]
    eigenvalues: torch.Tensor
    components: Optional[torch.Tensor]
    n_fit: torch.Tensor
    sweeps: torch.Tensor


def default_rank_tol(K: int) -> float:
    """32 K 2^-52: the backward error of the eigensolver relative to the largest eigenvalue."""
    return 32.0 * K * 2.0 ** -52


def check_rank_tol(rank_tol) -> float:
    """None or a value <= 0: 0.0 (the library's default); otherwise a float below 1."""
    if rank_tol is None:
        return 0.0
    tol = float(rank_tol)
    if math.isnan(tol) or tol >= 1.0:
        raise ValueError(f"rank_tol must be below 1, got {rank_tol!r}.")
    return max(tol, 0.0)


def check_components(A, K: int) -> int:
    """The number of components as an int: an integer with 1 <= A <= K."""
    if isinstance(A, bool) or not isinstance(A, (int, np.integer)) or not 1 <= A <= K:
        raise ValueError(f"A must be an integer with 1 <= A <= K = {K}, got {A!r}.")
    return int(A)


def pcr_fit_batched(XTX: torch.Tensor, XTY: Optional[torch.Tensor], A: int, *, return_components: bool = False,
                    rank_tol: Optional[float] = None, check: bool = False) -> PCRFit:
    """Principal component regression for every fold: ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device tensors (the
    outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is taken as F = 1), ``A``
    components, 1 <= A <= K <= 512.  ``XTY=None``: PCA only -- ``B`` is None and the components are returned.

    ``rank_tol`` (None: 32 K 2^-52): eigenvalues at or below ``rank_tol`` times the largest count as zero.
    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``sweeps`` once and
    raises ``numpy.linalg.LinAlgError`` naming the first fold that did not converge."""
    if not (isinstance(XTX, torch.Tensor) and XTX.is_cuda
            and (XTY is None or (isinstance(XTY, torch.Tensor) and XTY.is_cuda))):
        raise TypeError("pcr_fit_batched takes device tensors (the batched training matrices).")
    if XTX.dim() == 2:
        XTX = XTX.unsqueeze(0)
        if XTY is not None:
            XTY = XTY.unsqueeze(0) if XTY.dim() == 2 else XTY.reshape(1, -1, 1)
    if XTX.dim() != 3 or XTX.shape[1] != XTX.shape[2]:
        raise ValueError("XTX must be (F,K,K).")
    if XTY is not None:
        if XTY.dim() != 3 or XTY.shape[:2] != XTX.shape[:2]:
            raise ValueError("XTX must be (F,K,K) and XTY (F,K,M).")
        if XTX.dtype != XTY.dtype:
            raise ValueError("XTX and XTY must both be float64 or both float32.")
        if XTX.device != XTY.device:
            raise ValueError("XTX and XTY must be on one device.")
    if XTX.dtype not in (torch.float64, torch.float32):
        raise ValueError("XTX and XTY must both be float64 or both float32.")
    F, K = XTX.shape[:2]
    M = 0 if XTY is None else XTY.shape[2]
    if not 1 <= K <= MAX_K:
        raise ValueError(f"The device PCR takes 1 <= K <= {MAX_K}.")
    if XTY is not None and not 1 <= M <= MAX_RESPONSES:
        raise ValueError(f"The device PCR takes 1 to {MAX_RESPONSES} responses.")
    A = check_components(A, K)
    tol = check_rank_tol(rank_tol)
    want_V = return_components or XTY is None
    XTX = XTX.contiguous()
    if XTY is not None:
        XTY = XTY.contiguous()
    lib = _lib.load()
    dev = XTX.device
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    with torch.cuda.device(dev):
        one = lib.cvm_pcr_workspace_bytes(1, K, M, A)
        nbytes = min(lib.cvm_pcr_workspace_bytes(F, K, M, A), max(one, WORKSPACE_LIMIT))
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        B = None if XTY is None else torch.empty((F, A, K, M), dtype=XTX.dtype, device=dev)
        eig = torch.empty((F, A), dtype=torch.float64, device=dev)
        V = torch.empty((F, K, A), dtype=XTX.dtype, device=dev) if want_V else None
        n_fit = torch.empty((F,), dtype=torch.int32, device=dev)
        sweeps = torch.empty((F,), dtype=torch.int32, device=dev)
        if F == 0:                # nothing to launch (and empty tensors have no address to hand over)
            return PCRFit(B, eig, V, n_fit, sweeps)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.cvm_pcr_fit(_lib.ptr(XTX), _lib.ptr(XTY), F, K, M, A, code, tol, _lib.ptr(B), _lib.ptr(eig),
                             _lib.ptr(V), _lib.ptr(n_fit), _lib.ptr(sweeps), _lib.ptr(ws), nbytes, stream)
        _lib.check(rc, "cvm_pcr_fit")
        ws.record_stream(torch.cuda.current_stream(dev))
        if check:
            host = sweeps.cpu().numpy()
            bad = np.flatnonzero(host == -1)
            if bad.size:
                raise np.linalg.LinAlgError(
                    f"pcr_fit_batched: fold {int(bad[0])} did not converge in {MAX_SWEEPS} Jacobi sweeps; "
                    f"{bad.size} fold(s) failed.")
    return PCRFit(B, eig, V, n_fit, sweeps)
