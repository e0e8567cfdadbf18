"""Elastic net and lasso over a grid of penalties on the training matrices of a batch of folds, on the device:
for fold f, response m and penalty l, with ``G = XTX[f]``, ``h = XTY[f][:, m]`` and ``rho = l1_ratio``,

    B[f, l, :, m] = argmin over beta of  1/2 beta' G beta - h' beta + lambda_l (rho |beta|_1 + 1/2 (1 - rho) |beta|_2^2)

by one launch of ``cvm_enet_fit`` (include/cvmhip.h) -- cyclic coordinate descent with covariance updates in
float64, one wavefront per (fold, response), the penalties of a path walked from the largest down with warm starts.

The problem is stated on the training matrices as they are, with whatever centring and scaling the ``CVMatrix``
applied.  For unweighted, centred data of ``n`` training rows it is scikit-learn's
``ElasticNet(alpha=lambda / n, l1_ratio=rho, fit_intercept=False)``; with weights, the sum of the training
weights takes the place of ``n``.

The coefficients have the layout ``pls_validation_sse`` scores, with lambda in place of the number of
components.  No CPU fallback."""

from __future__ import annotations

import warnings
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._stage import check_fit_dims, check_grid, dtype_code, launch, training_pair

MAX_K = 4096
MAX_RESPONSES = 64
MAX_PENALTIES = 256
CONVERGED, MAX_SWEEPS_REACHED, NOT_FINITE = 0, 1, 2


class EnetFit(NamedTuple):
    """``B`` (F, L, K, M) in the dtype of XTX: ``B[f, l]`` = coefficients of fold f with penalty ``lambdas[l]``.
    ``info`` (F, L, M) int32 on the device: 0 converged (the KKT violation of every coordinate, from a freshly
    formed ``h - G beta``, is at most ``tol * max|h|``); 1 ``max_sweeps`` reached, ``B[f, l, :, m]`` is the last
    iterate; 2 a value that is not finite was met, ``B[f, l, :, m]`` is all NaN.  ``sweeps`` (F, L, M) int32 on
    the device: passes over the coordinates plus certificate passes."""
    B: torch.Tensor
    info: torch.Tensor
    sweeps: torch.Tensor


class EnetConvergenceWarning(RuntimeWarning):
    """Some problems reached ``max_sweeps`` without a passed optimality certificate."""


def check_lambdas(lambdas) -> np.ndarray:
    """The penalty grid as a contiguous 1-D float64 array: 1 to 256 values, each finite and > 0."""
    return check_grid("lambdas", lambdas, MAX_PENALTIES, low_open=True)


def check_solver_arguments(l1_ratio, tol, max_sweeps):
    """``(l1_ratio, tol, max_sweeps)`` as (float, float, int), or ValueError."""
    l1_ratio, tol = float(l1_ratio), float(tol)
    if l1_ratio == 0.0:
        raise ValueError("l1_ratio = 0 is ridge regression: use ridge_fit_batched.")
    if not 0.0 < l1_ratio <= 1.0:
        raise ValueError(f"l1_ratio must be in (0, 1], got {l1_ratio!r}.")
    if not 1e-12 <= tol < 1.0:
        raise ValueError(f"tol must be in [1e-12, 1), got {tol!r}.")
    if int(max_sweeps) != max_sweeps or max_sweeps < 1:
        raise ValueError(f"max_sweeps must be an integer >= 1, got {max_sweeps!r}.")
    return l1_ratio, tol, int(max_sweeps)


def enet_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, lambdas, l1_ratio: float = 0.5, *, tol: float = 1e-8,
                     max_sweeps: int = 1000, check: bool = False) -> EnetFit:
    """Elastic net coefficients for every fold, response and penalty: ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device
    tensors (the outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,M) or (K,) is taken as F = 1),
    ``lambdas`` anything ``np.asarray`` turns into a 1-D float64 array of positive values, in any order.

    The objective is the one of the module docstring; in scikit-learn's terms ``alpha = lambda / n`` with ``n``
    the number (sum of weights) of the training rows.  ``tol`` bounds the KKT violation relative to ``max|h|``;
    ``max_sweeps`` bounds the passes per problem.  Both defaults are interface choices, not measurements.

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``info`` once, raises
    ``numpy.linalg.LinAlgError`` for a problem of status 2 and warns (``EnetConvergenceWarning``, a
    ``RuntimeWarning``) naming the first (fold, lambda, response) of status 1."""
    lam = check_lambdas(lambdas)
    l1_ratio, tol, max_sweeps = check_solver_arguments(l1_ratio, tol, max_sweeps)
    XTX, XTY, F, K, M = training_pair("enet_fit_batched", XTX, XTY)
    check_fit_dims("The device elastic net", K, M, MAX_K, MAX_RESPONSES)
    L = lam.size
    dev = XTX.device
    B = torch.empty((F, L, K, M), dtype=XTX.dtype, device=dev)
    info = torch.empty((F, L, M), dtype=torch.int32, device=dev)
    sweeps = torch.empty((F, L, M), dtype=torch.int32, device=dev)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return EnetFit(B, info, sweeps)
    lib = _lib.load()
    launch("cvm_enet_fit", dev,
           lambda ws, nbytes, stream: lib.cvm_enet_fit(
               _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, lam.ctypes.data, L, l1_ratio, tol, max_sweeps,
               dtype_code(XTX.dtype), _lib.ptr(B), _lib.ptr(info), _lib.ptr(sweeps), ws, nbytes, stream),
           lib.cvm_enet_workspace_bytes(F, K, M, L))
    if check:
        host = info.cpu().numpy()
        bad = np.argwhere(host == NOT_FINITE)
        if bad.size:
            f, l, m = (int(v) for v in bad[0])
            raise np.linalg.LinAlgError(
                f"enet_fit_batched: fold {f}, lambda[{l}] = {lam[l]!r}, response {m}: a value that is not finite "
                f"was met; {len(bad)} problem(s) failed.")
        slow = np.argwhere(host == MAX_SWEEPS_REACHED)
        if slow.size:
            f, l, m = (int(v) for v in slow[0])
            warnings.warn(
                f"enet_fit_batched: fold {f}, lambda[{l}] = {lam[l]!r}, response {m}: no optimality certificate "
                f"after max_sweeps = {max_sweeps}; {len(slow)} problem(s) did not converge.",
                EnetConvergenceWarning, stacklevel=2)
    return EnetFit(B, info, sweeps)


def lasso_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, lambdas, *, tol: float = 1e-8, max_sweeps: int = 1000,
                      check: bool = False) -> EnetFit:
    """``enet_fit_batched`` with ``l1_ratio = 1``: ``alpha = lambda / n`` of scikit-learn's ``Lasso``."""
    return enet_fit_batched(XTX, XTY, lambdas, 1.0, tol=tol, max_sweeps=max_sweeps, check=check)


def _xty3(XTY: torch.Tensor) -> torch.Tensor:
    if not isinstance(XTY, torch.Tensor) or XTY.dim() not in (1, 2, 3):
        raise ValueError("XTY must be a tensor (F,K,M), (K,M) or (K,).")
    if XTY.dim() == 1:
        return XTY.reshape(1, -1, 1)
    return XTY.unsqueeze(0) if XTY.dim() == 2 else XTY


def lambda_max(XTY: torch.Tensor, l1_ratio: float) -> torch.Tensor:
    """(F, M): the smallest penalty whose solution is all zero, ``max_j |h_j| / l1_ratio``, per fold and
    response.  Plain torch on the tensor's own device; no synchronisation."""
    l1_ratio = check_solver_arguments(l1_ratio, 1e-8, 1)[0]
    return _xty3(XTY).abs().amax(dim=1) / l1_ratio


def lambda_grid(XTY: torch.Tensor, l1_ratio: float, n: int = 20, eps: float = 1e-3) -> np.ndarray:
    """``n`` penalties, log-spaced downwards from the largest ``lambda_max`` over folds and responses to ``eps``
    times it (float64, descending).  One read-back of one number."""
    if int(n) != n or not 1 <= n <= MAX_PENALTIES:
        raise ValueError(f"n must be an integer in 1 .. {MAX_PENALTIES}, got {n!r}.")
    if not 0.0 < eps < 1.0:
        raise ValueError(f"eps must be in (0, 1), got {eps!r}.")
    lm = lambda_max(XTY, l1_ratio)
    if lm.numel() == 0:
        raise ValueError("lambda_grid needs at least one fold and one response.")
    top = float(lm.double().max().item())
    if not np.isfinite(top) or top <= 0.0:
        raise ValueError(f"the largest lambda_max is {top!r}: no grid below it.")
    return top * np.logspace(0.0, np.log10(eps), int(n)) if n > 1 else np.array([top])
