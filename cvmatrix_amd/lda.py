"""Linear discriminant analysis with shrinkage on the training matrices of a batch of folds, on the device.
With ``h_c = XTY[f][:, c]`` (the class sums of the centred X), ``n_c`` the training weight of class c,
``n = sum_c n_c`` and ``m_c = h_c / n_c``::

    S_w     = XTX[f] - sum_c h_c h_c^T / n_c                 within-class scatter
    Sigma_g = (1 - g) S_w / n + g (tr S_w / (n K)) I          shrunk pooled covariance
    delta_c(z) = z^T Sigma_g^-1 m_c - 1/2 m_c^T Sigma_g^-1 m_c + log(n_c / n)

for every fold and every shrinkage g, by one call of ``cvm_lda_fit`` (include/cvmhip.h): a rank-C downdate of
every fold's XTX and the Cholesky solve of the device ridge, in float64.  This is scikit-learn's
``LinearDiscriminantAnalysis(solver="lsqr", shrinkage=g)`` up to a term common to all classes.  No row of X is
read to fit the models; ``lda_cv_decision`` scores them with one ``cv_predict``.  No CPU fallback."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._stage import check_grid, dtype_code, launch, training_pair
from .predict import cv_predict

MAX_K = 4096
MIN_CLASSES = 2
MAX_CLASSES = 64
MAX_SHRINKAGES = 256
WORKSPACE_LIMIT = 4 << 30     # bytes; fewer folds and factorisations run at once beyond it (same results to the bit)


class LDAFit(NamedTuple):
    """``coef`` (F, L, K, C) and ``intercept`` (F, L, C) in the dtype of XTX: the discriminants of fold f with
    ``shrinkage[l]`` for a row z standardised by the fold's statistics are ``z @ coef[f, l] + intercept[f, l]``.
    ``priors`` (F, C) float64: ``class_weights / n``.  ``info`` (F, L) int32 on the device: 0; j > 0 where pivot j
    of the factorisation was not positive (a singular within-class scatter at shrinkage 0); -1 where the fold
    holds a value that is not finite, a negative class weight or a within-class scatter without a positive
    trace.  Where ``info != 0``, ``coef[f, l]`` and ``intercept[f, l]`` are NaN.  A class absent from a fold's
    training set has ``coef`` 0, ``intercept`` -inf and ``priors`` 0 there: it is never predicted."""
    coef: torch.Tensor
    intercept: torch.Tensor
    priors: torch.Tensor
    info: torch.Tensor


def check_shrinkage(shrinkage) -> np.ndarray:
    """The shrinkage grid as a contiguous 1-D float64 array: a scalar or 1 to 256 values, each in [0, 1]."""
    return check_grid("shrinkage", shrinkage, MAX_SHRINKAGES, low_open=False, high=1, scalar_ok=True)


def check_dims(K: int, C: int) -> None:
    """1 <= K <= 4096 variables, 2 <= C <= 64 classes."""
    if not 1 <= K <= MAX_K:
        raise ValueError(f"The device LDA takes 1 <= K <= {MAX_K}, got {K}.")
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        raise ValueError(f"The device LDA takes {MIN_CLASSES} to {MAX_CLASSES} classes, got {C}.")


def check_class_weights(class_weights, F: int, C: int, dev) -> torch.Tensor:
    """The class weights as a contiguous (F, C) float64 tensor on ``dev`` ((C,) is taken as F = 1)."""
    if not isinstance(class_weights, torch.Tensor):
        raise TypeError("class_weights must be a device tensor (F, C) of float64.")
    if class_weights.dim() == 1 and F == 1:
        class_weights = class_weights.unsqueeze(0)
    if tuple(class_weights.shape) != (F, C) or class_weights.dtype != torch.float64:
        raise ValueError(f"class_weights must be ({F}, {C}) float64, got {tuple(class_weights.shape)} "
                         f"{class_weights.dtype}.")
    if class_weights.device != dev:
        raise ValueError(f"XTX, XTY and class_weights must be on one device (class_weights on "
                         f"{class_weights.device}, the matrices on {dev}).")
    return class_weights.contiguous()


def training_class_weights(cvm, folds) -> torch.Tensor:
    """(F, C) float64 on the device: per fold, the training sum of ``w * Y[:, c]`` -- the total minus the fold's
    validation rows.  ``cvm``: a fitted ``CVMatrix`` with the 0/1 class indicator as Y; ``folds``: what
    ``training_XTX_XTY_batched`` is given.  Sums of 0/1 (times integer weights) are exact; every sum is a
    ``torch.sum`` over a fixed shape.  Never waits for the device."""
    if cvm.X is None or cvm.Y is None:
        raise ValueError("training_class_weights needs a CVMatrix fitted with Y (the class indicator).")
    batch = cvm.prepare_folds(folds)
    dev = cvm.X.device
    wY = cvm.Y.to(torch.float64)
    if cvm.weights is not None:
        wY = wY * cvm.weights.reshape(-1, 1).to(torch.float64)
    total = wY.sum(dim=0)
    F = batch.n_folds
    longest = int(batch.sizes.max()) if F else 0
    if longest == 0:
        return total.expand(F, -1).contiguous()
    # the validation rows of every fold as one (F, longest) gather, short folds padded with weight 0
    n_idx = int(batch.host_offsets[-1])
    pos = batch.offsets[:-1, None] + torch.arange(longest, dtype=torch.int64, device=dev)[None, :]
    valid = pos < batch.offsets[1:, None]
    rows = batch.idx[pos.clamp(max=n_idx - 1)]
    val = (wY[rows] * valid[..., None].to(torch.float64)).sum(dim=1)
    return total[None, :] - val


def lda_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, class_weights: torch.Tensor, shrinkage=0.0, *,
                    check: bool = False) -> LDAFit:
    """Discriminants for every fold and every shrinkage: ``XTX`` (F,K,K) / ``XTY`` (F,K,C) device tensors (the
    outputs of ``training_XTX_XTY_batched``; a single (K,K) with (K,C) is taken as F = 1), ``class_weights``
    (F,C) -- or (C,) for F = 1 -- float64 on the same device (``training_class_weights``), ``shrinkage`` a scalar
    or anything ``np.asarray`` turns into a 1-D float64 array with values in [0, 1].  K <= 4096, 2 <= C <= 64,
    at most 256 shrinkage values.

    Preconditions that cannot be seen from the tensors: X is centred on the training set (``center_X``); Y is a
    0/1 indicator with one 1 per row; Y is not scaled (centring Y or not gives the same XTY once X is centred).

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``info`` once and raises
    ``numpy.linalg.LinAlgError`` naming the first failed (fold, shrinkage)."""
    g = check_shrinkage(shrinkage)
    XTX, XTY, F, K, C = training_pair("lda_fit_batched", XTX, XTY)
    check_dims(K, C)
    dev = XTX.device
    cw = check_class_weights(class_weights, F, C, dev)
    L = g.size
    coef = torch.empty((F, L, K, C), dtype=XTX.dtype, device=dev)
    intercept = torch.empty((F, L, C), dtype=XTX.dtype, device=dev)
    info = torch.empty((F, L), dtype=torch.int32, device=dev)
    priors = cw / cw.sum(dim=1, keepdim=True)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return LDAFit(coef, intercept, priors, info)
    lib = _lib.load()
    # the smallest workspace: one fold record and one factorisation (include/cvmhip.h)
    one = (lib.cvm_lda_workspace_bytes(1, K, C, L) - lib.cvm_ridge_workspace_bytes(1, K, C, L)
           + lib.cvm_ridge_workspace_bytes(1, K, C, 1))
    launch("cvm_lda_fit", dev,
           lambda ws, nbytes, stream: lib.cvm_lda_fit(
               _lib.ptr(XTX), _lib.ptr(XTY), _lib.ptr(cw), F, K, C, g.ctypes.data, L, dtype_code(XTX.dtype),
               _lib.ptr(coef), _lib.ptr(intercept), _lib.ptr(info), ws, nbytes, stream),
           lib.cvm_lda_workspace_bytes(F, K, C, L), one=one, limit=WORKSPACE_LIMIT)
    fit = LDAFit(coef, intercept, priors, info)
    if check:
        raise_on_failure(fit, g)
    return fit


def raise_on_failure(fit: LDAFit, shrinkage) -> None:
    """Read ``fit.info`` (one wait for the device) and raise ``numpy.linalg.LinAlgError`` naming the first
    failed (fold, shrinkage)."""
    g = check_shrinkage(shrinkage)
    host = fit.info.cpu().numpy()
    bad = np.argwhere(host != 0)
    if bad.size:
        f, l = (int(v) for v in bad[0])
        why = ("a value that is not finite, a negative class weight or a within-class scatter without a positive "
               "trace" if host[f, l] < 0 else
               f"pivot {int(host[f, l])} is not positive (the within-class scatter is singular: use shrinkage > 0)")
        raise np.linalg.LinAlgError(
            f"lda_fit_batched: fold {f}, shrinkage[{l}] = {g[l]!r}: {why}; {len(bad)} model(s) failed.")


def lda_cv_decision(cvm, folds, stats, fit: LDAFit, *, order: str = "rows") -> torch.Tensor:
    """The discriminants of every validation row under its own fold's models, (N, L, C) (``order="folds"``:
    (n_idx, L, C), as ``cv_predict`` orders them): ``cv_predict(cvm, folds, (muX, sdX, None, None), fit.coef)``
    plus the intercept of the fold that holds the row, gathered on the device.  ``stats``: the statistics tuple
    of ``training_XTX_XTY_batched`` (its Y side is not used).  Rows in no fold are NaN.  Never waits for the
    device."""
    if len(stats) != 4:
        raise ValueError("stats must be (muX, sdX, muY, sdY).")
    batch = cvm.prepare_folds(folds)
    scores = cv_predict(cvm, batch, (stats[0], stats[1], None, None), fit.coef, order=order)
    n_idx = int(batch.host_offsets[-1])
    if n_idx == 0:
        return scores
    dev = scores.device
    fold_of = torch.searchsorted(batch.offsets[1:], torch.arange(n_idx, dtype=torch.int64, device=dev), right=True)
    if order == "folds":
        return scores + fit.intercept[fold_of]
    # (rows in no fold keep the NaN cv_predict gave them)
    return scores.index_add_(0, batch.idx, fit.intercept[fold_of])


def lda_cv_predict(cvm, folds, stats, fit: LDAFit, *, order: str = "rows") -> torch.Tensor:
    """The predicted class of every validation row per shrinkage, int64 (N, L): the argmax of ``lda_cv_decision``;
    -1 for rows in no fold (and under a model that failed: ``fit.info``)."""
    d = lda_cv_decision(cvm, folds, stats, fit, order=order)
    labels = d.argmax(dim=2)
    return torch.where(torch.isnan(d[:, :, 0]), torch.full_like(labels, -1), labels)


def cv_lda(cvm, folds, shrinkage=0.0):
    """Fold stage, class weights and ``lda_fit_batched`` in one call: ``(fit, stats)``, ``stats`` being the
    statistics tuple ``lda_cv_decision`` and ``lda_cv_predict`` take.  The one place the model's flags are
    checked: raises ``ValueError`` unless ``center_X`` is set and ``scale_Y`` is not."""
    if not cvm.center_X:
        raise ValueError("cv_lda needs a CVMatrix with center_X=True: the class sums must be sums of centred rows.")
    if cvm.scale_Y:
        raise ValueError("cv_lda needs a CVMatrix with scale_Y=False: Y is the 0/1 class indicator.")
    check_shrinkage(shrinkage)
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    fit = lda_fit_batched(XTX, XTY, training_class_weights(cvm, batch), shrinkage)
    return fit, stats
