"""Improved Kernel PLS (algorithm #2 of Dayal & MacGregor 1997) on the training matrices of a
batch of folds, on the device -- the step after the cvmatrix hot path.

The reference names its consumer (README.md:23, cvmatrix/partitioner.py:27-31): the ``ikpls``
package runs this algorithm on every fold's ``(XTX, XTY)``.  Here the matrices stay where
``CVMatrix.training_XTX_XTY_batched`` wrote them (HBM) and one launch of ``cvm_pls_fit``
(include/cvmhip.h) fits all folds.  No CPU fallback."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._stage import dtype_code, launch, model_batch, training_pair

MAX_RESPONSES = 64
MAX_COMPONENTS = 512


class PLSFit(NamedTuple):
    """``B`` (F,A,K,M): ``B[f, a]`` = regression coefficients with ``a + 1`` components;
    ``W, P, R`` (F,K,A) and ``Q`` (F,M,A) when requested, else None; ``n_fit`` (F,) int32:
    components extracted per fold (less than A only when XTY deflated to zero: the components
    beyond are exactly zero).  A fold whose XTX or XTY holds a NaN or an infinity has ``n_fit`` -1
    and NaN in every component of ``B, W, P, Q, R``."""
    B: torch.Tensor
    W: Optional[torch.Tensor]
    P: Optional[torch.Tensor]
    Q: Optional[torch.Tensor]
    R: Optional[torch.Tensor]
    n_fit: torch.Tensor


def pls_plan(n_folds: int, K: int, M: int, A: int, dtype=np.float64) -> dict:
    """How a problem is cut: row slices per fold, rows per slice, folds per launch, whether the
    slice of XTX stays in LDS (host logic only: runs without a GPU)."""
    lib = _lib.load()
    info = np.zeros(5, dtype=np.int64)
    code = _lib.CVM_F64 if np.dtype(dtype) == np.float64 else _lib.CVM_F32
    _lib.check(lib.cvm_pls_plan(n_folds, K, M, A, code, info.ctypes.data), "cvm_pls_plan")
    return {"slices": int(info[0]), "rows": int(info[1]), "folds_per_launch": int(info[2]),
            "xtx_in_lds": int(info[3]) == 1, "lds_bytes": int(info[4]),
            "kernel": "replicated small state, one barrier per component" if int(info[3]) == 2
            else ("row slices, four barriers per component" if int(info[0]) > 1 else "one workgroup per fold")}


def pls_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, A: int, *, return_factors: bool = False,
                    check: bool = True) -> PLSFit:
    """Fit A-component PLS models on ``XTX`` (F,K,K) / ``XTY`` (F,K,M) device tensors (the
    outputs of ``training_XTX_XTY_batched``; a single (K,K)/(K,M) pair is taken as F = 1).

    The routes that cut a fold into slices need an otherwise idle device (the slices of a fold wait for each
    other; ``CVM_PLS_NO_REP`` opts out of the one-barrier route).  If a slice finds no place to run, the
    barrier times out and the library recomputes every fold with one workgroup per fold in the same call;
    only where a fold does not fit one workgroup's LDS are the outputs overwritten with NaN (``n_fit`` -1) --
    ``check=True`` synchronises once to turn that case into an exception.  Nothing half-written is ever
    returned.

    Non-finite input: a fold with a NaN or an infinity anywhere in its ``XTX`` or ``XTY`` (what the fold stage
    hands over for a fold it could not compute) comes back as NaN in every component of ``B, W, P, Q, R`` with
    ``n_fit`` -1 -- never as zeros or other finite numbers, so ``pls_validation_sse`` and ``cv_rmse`` turn it
    into NaN errors, not into the finite error of predicting the training mean.  The status stays 0 (no
    exception) and every other fold has the bits it has when that fold is clean."""
    XTX, XTY, F, K, M = training_pair("pls_fit_batched", XTX, XTY)
    A = int(A)
    if not 1 <= A <= MAX_COMPONENTS:
        raise ValueError(f"A must be in [1, {MAX_COMPONENTS}].")
    if not 1 <= M <= MAX_RESPONSES:
        raise ValueError(f"The device PLS takes at most {MAX_RESPONSES} responses.")
    lib = _lib.load()
    dev, code = XTX.device, dtype_code(XTX.dtype)
    nbytes = lib.cvm_pls_workspace_bytes(F, K, M, A, code)
    if nbytes == 0 and F:
        raise ValueError("K is too large for the device PLS kernel.")
    B = torch.empty((F, A, K, M), dtype=XTX.dtype, device=dev)
    n_fit = torch.empty((F,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    W = P = Q = R = None
    if return_factors:
        W = torch.empty((F, K, A), dtype=XTX.dtype, device=dev)
        P = torch.empty_like(W)
        R = torch.empty_like(W)
        Q = torch.empty((F, M, A), dtype=XTX.dtype, device=dev)
    if F:                         # (no folds: nothing to launch, and empty tensors have no address to hand over)
        launch("cvm_pls_fit", dev,
               lambda ws, ws_bytes, stream: lib.cvm_pls_fit(
                   _lib.ptr(XTX), _lib.ptr(XTY), F, K, M, A, code, _lib.ptr(B), _lib.ptr(W), _lib.ptr(P), _lib.ptr(Q),
                   _lib.ptr(R), _lib.ptr(n_fit), _lib.ptr(status), ws, ws_bytes, stream),
               nbytes)
    # status 0: fine; 2: a barrier of the sliced launch timed out (a slice was not resident: another
    # stream's kernel on the device, a masked CU) and the library recomputed every fold with the kernel that
    # waits for nobody -- the outputs are valid; 1: it could not (a fold does not fit one workgroup's LDS):
    # the outputs are NaN / n_fit -1
    if check:
        st_ = int(status.item()) if F else 0
        pls_fit_batched.last_status = st_          # (0 or 2 after a successful call: tests, diagnostics)
        if st_ == 1:
            raise RuntimeError("cvm_pls_fit: workgroups of a fold were not co-resident (barrier timed out).")
    return PLSFit(B, W, P, Q, R, n_fit)


pls_fit_batched.last_status = None


def pls_validation_sse(cvm, folds, stats, B: torch.Tensor):
    """Weighted squared prediction errors of every fold's linear models on the fold's own validation rows,
    on the device (``cvm_pls_validation_sse``): ``cvm`` a fitted ``CVMatrix`` with Y, ``folds`` what
    ``training_XTX_XTY_batched`` was given (a ``Partitioner``, index arrays or a ``FoldBatch``), ``stats``
    the statistics tuple that call returned (each None, (F, 1, width) or (F, width), as ``cv_predict`` takes them), ``B`` any (F,A,K,M) stack of coefficients: ``pls_fit_batched``'s
    (A components) or ``ridge.ridge_fit_batched(...).B`` (A = the penalties of the grid).  Returns
    ``(sse, wsum)``: float64 tensors (F,A,M) and (F,) -- the cross-validated RMSE with ``a + 1``
    components is ``sqrt(sse.sum(0)[a] / wsum.sum())`` (``cv_rmse``)."""
    if cvm.X is None or cvm.Y is None:
        raise ValueError("pls_validation_sse needs a CVMatrix fitted with Y.")
    # (the kernel reads X and Y at the row strides K and M)
    if cvm._Kd != cvm._Ku or (cvm._Md or 0) != (cvm._Mu or 0):
        raise ValueError("pls_validation_sse takes device results of an unpadded float32 / float64 model "
                         "(K even, float64: M even, or copy=False).")
    batch, B, (muX, sdX, muY, sdY), max_rows = model_batch("pls_validation_sse", cvm, folds, stats, B)
    F, A, K, M = B.shape
    if M != cvm.M:
        raise ValueError("B does not belong to these folds / this model.")
    lib = _lib.load()
    dev = B.device
    sse = torch.empty((F, A, M), dtype=torch.float64, device=dev)
    wsum = torch.empty((F,), dtype=torch.float64, device=dev)
    launch("cvm_pls_validation_sse", dev,
           lambda ws, nbytes, stream: lib.cvm_pls_validation_sse(
               _lib.ptr(cvm.X), _lib.ptr(cvm.Y), _lib.ptr(cvm.weights), _lib.ptr(batch.idx), _lib.ptr(batch.offsets),
               F, max_rows, K, M, A, dtype_code(B.dtype), _lib.ptr(muX), _lib.ptr(sdX), _lib.ptr(muY), _lib.ptr(sdY),
               _lib.ptr(B), _lib.ptr(sse), _lib.ptr(wsum), ws, nbytes, stream),
           lib.cvm_pls_sse_workspace_bytes(F, max_rows, M, A))
    return sse, wsum


def cv_rmse(sse: torch.Tensor, wsum: torch.Tensor) -> torch.Tensor:
    """(A, M) cross-validated RMSE per number of components and response from ``pls_validation_sse``."""
    return torch.sqrt(sse.sum(dim=0) / wsum.sum())
