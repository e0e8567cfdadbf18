"""Orthogonal matching pursuit -- greedy forward variable selection -- on the training matrices of a batch of
folds, on the device: for fold f and response m, with ``G = XTX[f]`` and ``h = XTY[f][:, m]``, the variables are
selected one at a time by the largest ``|h - G[:, S] gamma|`` (``normalize=True``: divided by ``sqrt(G_kk)``, the
correlation with the residual) and the coefficients on the selected set are refitted by least squares after every
selection, by one launch of ``cvm_omp_fit`` (include/cvmhip.h) -- a growing Cholesky factor in float64, one
wavefront per (fold, response).  With ``normalize=False`` this is scikit-learn's ``orthogonal_mp_gram``; each
response selects its own variables.

The coefficients have the layout ``pls_validation_sse`` scores, with the number of selected variables in place
of the number of components: ``pls_validation_sse(cvm, folds, stats, fit.B)`` and ``cv_rmse`` give the
cross-validated RMSE per number of variables.  No CPU fallback."""

from __future__ import annotations

import warnings
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._stage import check_count, check_fit_dims, check_tolerance, dtype_code, launch, training_pair

MAX_K = 4096
MAX_RESPONSES = 64
MAX_SELECTED = 64             # one lane of the wavefront per selected variable
WORKSPACE_LIMIT = 4 << 30     # bytes; fewer paths run at once beyond it (same results to the bit)


class OMPFit(NamedTuple):
    """``B`` (F, A, K, M) in the dtype of XTX: ``B[f, a, :, m]`` = the least-squares coefficients of fold f,
    response m on its first a+1 selected variables, exactly 0 elsewhere; for ``a >= n_fit[f, m]`` it repeats
    ``B[f, n_fit - 1, :, m]`` (all zeros if ``n_fit`` is 0).  ``support`` (F, A, M) int32 on the device: the index
    selected at step a, -1 for ``a >= n_fit``.  ``n_fit`` (F, M) int32 on the device: the variables selected, 0 .. A
    (fewer than A where the best remaining candidate was numerically dependent on the selected ones, or nothing
    was left to explain); -1 where a value that is not finite was met: ``B[f, :, :, m]`` is then all NaN and
    ``support[f, :, m]`` all -1."""
    B: torch.Tensor
    support: torch.Tensor
    n_fit: torch.Tensor


class OMPRankWarning(RuntimeWarning):
    """Some paths ended before ``n_nonzero`` variables were selected."""


def default_rank_tol(A: int) -> float:
    """32 A 2^-52: the backward error of a Cholesky factor of A variables relative to the diagonal."""
    return 32.0 * A * 2.0 ** -52


def check_rank_tol(rank_tol) -> float:
    """None or a value <= 0: 0.0 (the library's default); otherwise a float below 1."""
    return check_tolerance("rank_tol", rank_tol)


def check_selected(A, K: int) -> int:
    """The number of variables to select as an int: an integer with 1 <= A <= min(K, 64)."""
    top = min(K, MAX_SELECTED)
    return check_count("n_nonzero", A, top, f"min(K, {MAX_SELECTED}) = {top}")


def omp_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, n_nonzero: int, *, normalize: bool = False,
                    rank_tol: Optional[float] = None, check: bool = False) -> OMPFit:
    """Forward selection of up to ``n_nonzero`` variables for every fold and response: ``XTX`` (F,K,K) / ``XTY``
    (F,K,M) device tensors (the outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is
    taken as F = 1), 1 <= n_nonzero <= min(K, 64), K <= 4096, M <= 64.

    ``normalize=False`` selects by ``|alpha_k|`` (scikit-learn's rule), ``True`` by ``|alpha_k| / sqrt(G_kk)``;
    among equal scores the lowest index wins.  ``rank_tol`` (None: 32 n_nonzero 2^-52): a candidate whose
    Cholesky pivot is at or below ``rank_tol * G_jj`` ends the path.

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``n_fit`` once, raises
    ``numpy.linalg.LinAlgError`` naming the first (fold, response) that met a value that is not finite and warns
    (``OMPRankWarning``, a ``RuntimeWarning``) with the number of paths that ended early."""
    check_selected(n_nonzero, MAX_K)          # (what can be refused without the shapes is refused first)
    tol = check_rank_tol(rank_tol)
    XTX, XTY, F, K, M = training_pair("omp_fit_batched", XTX, XTY)
    check_fit_dims("The device OMP", K, M, MAX_K, MAX_RESPONSES)
    A = check_selected(n_nonzero, K)
    dev = XTX.device
    B = torch.empty((F, A, K, M), dtype=XTX.dtype, device=dev)
    support = torch.empty((F, A, M), dtype=torch.int32, device=dev)
    n_fit = torch.empty((F, M), dtype=torch.int32, device=dev)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return OMPFit(B, support, n_fit)
    lib = _lib.load()
    launch("cvm_omp_fit", dev,
           lambda ws, nbytes, stream: lib.cvm_omp_fit(
               _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, A, int(bool(normalize)), tol, dtype_code(XTX.dtype),
               _lib.ptr(B), _lib.ptr(support), _lib.ptr(n_fit), ws, nbytes, stream),
           lib.cvm_omp_workspace_bytes(F, K, M, A), one=lib.cvm_omp_workspace_bytes(1, K, 1, A),
           limit=WORKSPACE_LIMIT)
    if check:
        host = n_fit.cpu().numpy()
        bad = np.argwhere(host < 0)
        if bad.size:
            f, m = (int(v) for v in bad[0])
            raise np.linalg.LinAlgError(
                f"omp_fit_batched: fold {f}, response {m}: a value that is not finite was met; "
                f"{len(bad)} path(s) failed.")
        early = np.argwhere(host < A)
        if early.size:
            f, m = (int(v) for v in early[0])
            warnings.warn(
                f"omp_fit_batched: {len(early)} path(s) ended before {A} variables were selected (the first: "
                f"fold {f}, response {m}, after {int(host[f, m])}): the remaining candidates depend on the "
                f"selected variables or nothing was left to explain.", OMPRankWarning, stacklevel=2)
    return OMPFit(B, support, n_fit)
