"""PCA and principal component regression on the training matrices of a batch of folds, on the device:
the leading eigenpairs of every ``XTX[f]`` and the coefficients ``B[f, a] = sum_{j<=a} v_j (v_j^T XTY[f]) /
lambda_j`` with 1 .. A components, by one launch of ``cvm_pcr_fit`` (include/cvmhip.h) -- a cyclic Jacobi
eigensolver per fold in float64, K <= 512 -- or, with ``solver="blocked"``, by ``cvm_pcr_blocked_fit``: a cyclic
block Jacobi eigensolver with many workgroups per fold and its products on the matrix cores, K <= 4096, which
waits for the device once per sweep.

The coefficients have the layout ``pls_validation_sse`` scores: ``pls_validation_sse(cvm, folds, stats,
fit.B)`` and ``cv_rmse`` give the cross-validated RMSE per number of components.  No CPU fallback."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._stage import check_count, check_tolerance, dtype_code, launch, training_pair

MAX_K = 512
MAX_K_BLOCKED = 4096          # solver="blocked"
BLOCK = 32                    # the block size b of the blocked solver (PCRB_BLOCK in csrc/pcr_blocked.hpp)
SOLVERS = ("scalar", "blocked")
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
    return check_tolerance("rank_tol", rank_tol)


def check_components(A, K: int) -> int:
    """The number of components as an int: an integer with 1 <= A <= K."""
    return check_count("A", A, K, f"K = {K}")


def pcr_fit_batched(XTX: torch.Tensor, XTY: Optional[torch.Tensor], A: int, *, return_components: bool = False,
                    rank_tol: Optional[float] = None, check: bool = False, solver: str = "scalar",
                    max_sweeps: Optional[int] = None) -> PCRFit:
    """Principal component regression for every fold: ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device tensors (the
    outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is taken as F = 1), ``A``
    components, 1 <= A <= K <= 512 (4096 with ``solver="blocked"``).  ``XTY=None``: PCA only -- ``B`` is None and
    the components are returned.

    ``rank_tol`` (None: 32 K 2^-52): eigenvalues at or below ``rank_tol`` times the largest count as zero.
    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``sweeps`` once and
    raises ``numpy.linalg.LinAlgError`` naming the first fold that did not converge.

    ``solver="scalar"`` (the default): one workgroup per fold, one launch, no wait.  ``solver="blocked"``: the
    block Jacobi eigensolver, 1 <= K <= 4096, the same outputs under the same contract (not the same bits).  It
    WAITS FOR THE DEVICE ONCE PER SWEEP -- the host reads one word per fold to see which folds are done -- so it
    cannot run inside a graph capture.  ``max_sweeps`` (1 .. 60; None, the default, is 60; blocked solver only, a
    ``ValueError`` with the scalar one): a fold that has not converged by then is NaN with ``sweeps`` -1."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}.")
    blocked = solver == "blocked"
    if max_sweeps is None:
        max_sweeps = MAX_SWEEPS
    elif not blocked:
        raise ValueError("max_sweeps goes with solver='blocked' (the scalar solver always allows 60).")
    max_sweeps = check_count("max_sweeps", max_sweeps, MAX_SWEEPS, str(MAX_SWEEPS))
    limit = MAX_K_BLOCKED if blocked else MAX_K
    hint = "" if blocked else f" (solver='blocked' takes K up to {MAX_K_BLOCKED})"
    # (the order is a rule of the solver, not of the tensors: it is refused wherever the matrix lives)
    if isinstance(XTX, torch.Tensor) and XTX.dim() in (2, 3) and XTX.shape[-1] > limit:
        raise ValueError(f"The device PCR takes 1 <= K <= {limit}{hint}.")
    XTX, XTY, F, K, M = training_pair("pcr_fit_batched", XTX, XTY, y_optional=True)
    if not 1 <= K <= limit:
        raise ValueError(f"The device PCR takes 1 <= K <= {limit}{hint}.")
    if XTY is not None and not 1 <= M <= MAX_RESPONSES:
        raise ValueError(f"The device PCR takes 1 to {MAX_RESPONSES} responses.")
    A = check_components(A, K)
    tol = check_rank_tol(rank_tol)
    want_V = return_components or XTY is None
    dev = XTX.device
    B = None if XTY is None else torch.empty((F, A, K, M), dtype=XTX.dtype, device=dev)
    eig = torch.empty((F, A), dtype=torch.float64, device=dev)
    V = torch.empty((F, K, A), dtype=XTX.dtype, device=dev) if want_V else None
    n_fit = torch.empty((F,), dtype=torch.int32, device=dev)
    sweeps = torch.empty((F,), dtype=torch.int32, device=dev)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return PCRFit(B, eig, V, n_fit, sweeps)
    lib = _lib.load()
    if blocked:
        launch("cvm_pcr_blocked_fit", dev,
               lambda ws, nbytes, stream: lib.cvm_pcr_blocked_fit(
                   _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, A, dtype_code(XTX.dtype), tol, max_sweeps, _lib.ptr(B),
                   _lib.ptr(eig), _lib.ptr(V), _lib.ptr(n_fit), _lib.ptr(sweeps), ws, nbytes, stream),
               lib.cvm_pcr_blocked_workspace_bytes(F, K, M, A), one=lib.cvm_pcr_blocked_workspace_bytes(1, K, M, A),
               limit=WORKSPACE_LIMIT)
    else:
        launch("cvm_pcr_fit", dev,
               lambda ws, nbytes, stream: lib.cvm_pcr_fit(
                   _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, A, dtype_code(XTX.dtype), tol, _lib.ptr(B), _lib.ptr(eig),
                   _lib.ptr(V), _lib.ptr(n_fit), _lib.ptr(sweeps), ws, nbytes, stream),
               lib.cvm_pcr_workspace_bytes(F, K, M, A), one=lib.cvm_pcr_workspace_bytes(1, K, M, A),
               limit=WORKSPACE_LIMIT)
    if check:
        host = sweeps.cpu().numpy()
        bad = np.flatnonzero(host == -1)
        if bad.size:
            raise np.linalg.LinAlgError(
                f"pcr_fit_batched: fold {int(bad[0])} did not converge in {max_sweeps} Jacobi sweeps; "
                f"{bad.size} fold(s) failed.")
    return PCRFit(B, eig, V, n_fit, sweeps)
