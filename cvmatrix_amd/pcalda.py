"""PCA-LDA on the training matrices of a batch of folds, on the device: linear discriminant analysis on the
scores of the first 1, 2, .., A principal components of every fold -- the count-tuned sibling of the shrinkage
LDA of ``lda.py``, as PCR is ridge's.  With ``h_c = XTY[f][:, c]`` (the class sums of the centred X), ``n_c`` the
training weight of class c, ``n = sum_c n_c``, ``V`` (K, A) and ``lambda`` the leading eigenpairs of ``XTX[f]``::

    P = V^T H,  m~_c = p_c / n_c,  S = diag(lambda) - sum_c p_c p_c^T / n_c      (the scatter of the scores)
    S = L L^T column by column; the path ends before a component that does not exist or whose pivot d_j^2
        is not > pivot_tol lambda_j
    Z = L^-1 M~,  W = V L^-T
    coef[a] = coef[a-1] + n w_a z_a^T,   intercept[a] = intercept[a-1] - 1/2 n z_a o z_a

The Cholesky factor of a leading block is the leading block of the factor, so one A x A factorisation per fold
gives the models on 1 .. A components, by one call of ``cvm_pcalda_fit`` (include/cvmhip.h) behind
``pcr_fit_batched(..., return_components=True)``.  ``coef[f, a]``, ``intercept[f, a]`` are scikit-learn's
``Pipeline(PCA(a + 1), LinearDiscriminantAnalysis(solver="lsqr"))`` up to a term common to all classes.  The fit
has ``LDAFit``'s field names: ``lda_cv_decision`` and ``lda_cv_predict`` of ``lda.py`` score it as it is, with
components in place of shrinkages.  No row of X is read to fit the models.  No CPU fallback."""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._stage import check_count, check_tolerance, dtype_code, launch, training_pair
from .lda import MAX_CLASSES, MIN_CLASSES, check_class_weights, training_class_weights
from .pcr import MAX_K as MAX_K_SCALAR, MAX_K_BLOCKED, SOLVERS, pcr_fit_batched

MAX_K = 4096                  # cvm_pcalda_fit itself; the eigensolver in front of it may take less
MAX_COMPONENTS = 64           # the factor lies in LDS with one row per lane
DEFAULT_PIVOT_TOL = 2.0 ** -26
WORKSPACE_LIMIT = 4 << 30     # bytes; fewer folds run at once beyond it (same results to the bit)


class PCALDAFit(NamedTuple):
    """``coef`` (F, A, K, C) and ``intercept`` (F, A, C) in the dtype of XTX: the discriminants of fold f on its
    first a+1 principal components for a row z standardised by the fold's statistics are ``z @ coef[f, a] +
    intercept[f, a]``.  ``priors`` (F, C) float64: ``class_weights / n``.  ``n_fit`` (F,) int32 on the device: the
    models that exist; ``coef[f, a]`` and ``intercept[f, a]`` for ``a >= n_fit[f]`` repeat those of ``n_fit[f] - 1``
    (``n_fit`` 0: the prior-only model, ``coef`` 0 and ``intercept`` the log priors).  ``info`` (F,) int32: 0 all A
    models exist; 1 the path ended at the number of components that exist; 2 it ended at a pivot (no within-class
    variance left along the next component); -1 the fold is flagged (a value that is not finite, a negative
    class weight, no weight at all, an eigensolver that failed): ``n_fit`` -1 and NaN throughout.  ``eigenvalues``
    (F, A) float64, descending.  A class absent from a fold's training set has ``coef`` 0, ``intercept`` -inf and
    ``priors`` 0 there: it is never predicted."""
    coef: torch.Tensor
    intercept: torch.Tensor
    priors: torch.Tensor
    n_fit: torch.Tensor
    info: torch.Tensor
    eigenvalues: torch.Tensor


def check_pivot_tol(pivot_tol) -> float:
    """None or a value <= 0: 0.0 (the library's default, 2^-26); otherwise a float below 1."""
    return check_tolerance("pivot_tol", pivot_tol)


def check_components(A, K: Optional[int] = None) -> int:
    """The number of components as an int: an integer with 1 <= A <= min(K, 64) (K None: 1 <= A <= 64)."""
    top = MAX_COMPONENTS if K is None else min(K, MAX_COMPONENTS)
    return check_count("A", A, top, f"min(K, {MAX_COMPONENTS})" + ("" if K is None else f" = {top}"))


def check_dims(K: int, C: int, A, limit: int = MAX_K) -> int:
    """1 <= K <= limit variables, 2 <= C <= 64 classes, 1 <= A <= min(K, 64) components; returns A."""
    if not 1 <= K <= limit:
        raise ValueError(f"The device PCA-LDA takes 1 <= K <= {limit}, got {K}"
                         + (f" (solver='blocked' takes K up to {MAX_K_BLOCKED})." if limit < MAX_K_BLOCKED else "."))
    if not MIN_CLASSES <= C <= MAX_CLASSES:
        raise ValueError(f"The device PCA-LDA takes {MIN_CLASSES} to {MAX_CLASSES} classes, got {C}.")
    return check_components(A, K)


def _tensors(who: str, **named) -> None:
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a device tensor, got {type(t).__name__}.")


def _on_device(who: str, **named) -> None:
    for name, t in named.items():
        if not t.is_cuda:
            raise TypeError(f"{who} takes device tensors ({name} is on {t.device}).")


def pcalda_from_components(components: torch.Tensor, eigenvalues: torch.Tensor, n_comp: torch.Tensor,
                           XTY: torch.Tensor, class_weights: torch.Tensor, *, pivot_tol: Optional[float] = None,
                           check: bool = False) -> PCALDAFit:
    """The discriminants on 1 .. A components for every fold from eigenpairs that are already there:
    ``components`` (F, K, A) and ``XTY`` (F, K, C) device tensors of one dtype (float64 or float32; a single (K, A)
    with (K, C) is taken as F = 1), ``eigenvalues`` (F, A) float64 descending, ``n_comp`` (F,) int32 (the
    components that exist: ``PCRFit.n_fit``), ``class_weights`` (F, C) float64 (``training_class_weights``), all on
    one device.  1 <= K <= 4096, 2 <= C <= 64, 1 <= A <= min(K, 64).  ``pivot_tol`` (None: 2^-26): the path ends
    at the first component whose pivot is not above ``pivot_tol`` times its eigenvalue.

    ``check=False`` (the default) does not wait for the device.  ``check=True`` reads ``info`` once and raises
    ``numpy.linalg.LinAlgError`` naming the first flagged fold."""
    who = "pcalda_from_components"
    tol = check_pivot_tol(pivot_tol)
    _tensors(who, components=components, eigenvalues=eigenvalues, n_comp=n_comp, XTY=XTY, class_weights=class_weights)
    V = components
    if V.dim() == 2 and XTY.dim() == 2:
        V, XTY = V.unsqueeze(0), XTY.unsqueeze(0)
        eigenvalues = eigenvalues.reshape(1, -1) if eigenvalues.dim() == 1 else eigenvalues
        n_comp = n_comp.reshape(1) if n_comp.dim() == 0 else n_comp
    if V.dim() != 3 or XTY.dim() != 3 or XTY.shape[:2] != V.shape[:2]:
        raise ValueError("components must be (F,K,A) and XTY (F,K,C).")
    F, K, A = V.shape
    C = XTY.shape[2]
    check_dims(K, C, A)
    if V.dtype != XTY.dtype or V.dtype not in (torch.float64, torch.float32):
        raise ValueError("components and XTY must both be float64 or both float32.")
    dev = V.device
    if tuple(eigenvalues.shape) != (F, A) or eigenvalues.dtype != torch.float64:
        raise ValueError(f"eigenvalues must be ({F}, {A}) float64, got {tuple(eigenvalues.shape)} {eigenvalues.dtype}.")
    if tuple(n_comp.shape) != (F,) or n_comp.dtype != torch.int32:
        raise ValueError(f"n_comp must be ({F},) int32, got {tuple(n_comp.shape)} {n_comp.dtype}.")
    if XTY.device != dev or eigenvalues.device != dev or n_comp.device != dev:
        raise ValueError("components, eigenvalues, n_comp and XTY must be on one device.")
    cw = check_class_weights(class_weights, F, C, dev)
    _on_device(who, components=V)
    V, XTY, eig, n_comp = V.contiguous(), XTY.contiguous(), eigenvalues.contiguous(), n_comp.contiguous()
    coef = torch.empty((F, A, K, C), dtype=V.dtype, device=dev)
    intercept = torch.empty((F, A, C), dtype=V.dtype, device=dev)
    n_fit = torch.empty((F,), dtype=torch.int32, device=dev)
    info = torch.empty((F,), dtype=torch.int32, device=dev)
    priors = cw / cw.sum(dim=1, keepdim=True)
    fit = PCALDAFit(coef, intercept, priors, n_fit, info, eig)
    if F == 0:                    # nothing to launch (and empty tensors have no address to hand over)
        return fit
    lib = _lib.load()
    launch("cvm_pcalda_fit", dev,
           lambda ws, nbytes, stream: lib.cvm_pcalda_fit(
               _lib.ptr(V), _lib.ptr(eig), _lib.ptr(n_comp), _lib.ptr(XTY), _lib.ptr(cw), F, K, C, A,
               dtype_code(V.dtype), tol, _lib.ptr(coef), _lib.ptr(intercept), _lib.ptr(n_fit), _lib.ptr(info),
               ws, nbytes, stream),
           lib.cvm_pcalda_workspace_bytes(F, K, C, A), one=lib.cvm_pcalda_workspace_bytes(1, K, C, A),
           limit=WORKSPACE_LIMIT)
    if check:
        raise_on_failure(fit)
    return fit


def raise_on_failure(fit: PCALDAFit) -> None:
    """Read ``fit.info`` (one wait for the device) and raise ``numpy.linalg.LinAlgError`` naming the first
    flagged fold."""
    host = fit.info.cpu().numpy()
    bad = np.flatnonzero(host < 0)
    if bad.size:
        raise np.linalg.LinAlgError(
            f"pcalda: fold {int(bad[0])} is flagged: a value that is not finite, a negative class weight, no "
            f"weight at all or an eigensolver that failed; {bad.size} fold(s) flagged.")


def pcalda_fit_batched(XTX: torch.Tensor, XTY: torch.Tensor, class_weights: torch.Tensor, A: int, *,
                       solver: str = "scalar", rank_tol: Optional[float] = None, max_sweeps: Optional[int] = None,
                       pivot_tol: Optional[float] = None, check: bool = False) -> PCALDAFit:
    """PCA-LDA for every fold: ``XTX`` (F,K,K) / ``XTY`` (F,K,C) device tensors (the outputs of
    ``training_XTX_XTY_batched``; a single (K,K) with (K,C) is taken as F = 1), ``class_weights`` (F,C) -- or (C,)
    for F = 1 -- float64 on the same device (``training_class_weights``), ``A`` components, 1 <= A <= min(K, 64),
    2 <= C <= 64, K <= 512 (4096 with ``solver="blocked"``).

    ``pcr_fit_batched(XTX, None, A, return_components=True, solver=..., rank_tol=..., max_sweeps=...)`` gives the
    eigenpairs, ``pcalda_from_components`` the models; ``solver``, ``rank_tol`` and ``max_sweeps`` are the
    eigensolver's (pcr.py), ``pivot_tol`` and ``check`` the wrapper's.  The call waits for the device no more than
    the chosen eigensolver does (the scalar one: never; the blocked one: once per sweep).

    Preconditions that cannot be seen from the tensors: X is centred on the training set (``center_X``); Y is a
    0/1 indicator with one 1 per row; Y is not scaled."""
    who = "pcalda_fit_batched"
    A = check_components(A)
    check_pivot_tol(pivot_tol)
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}.")
    limit = MAX_K_BLOCKED if solver == "blocked" else MAX_K_SCALAR
    _tensors(who, XTX=XTX, XTY=XTY, class_weights=class_weights)
    # the rules of the shapes hold wherever the tensors live: they are refused before the device is asked for
    if XTX.dim() in (2, 3) and XTY.dim() == XTX.dim() and XTX.shape[-1] == XTX.shape[-2] == XTY.shape[-2]:
        F = 1 if XTX.dim() == 2 else XTX.shape[0]
        check_dims(XTX.shape[-1], XTY.shape[-1], A, limit)
        check_class_weights(class_weights, F, XTY.shape[-1], XTX.device)
    XTX, XTY, F, K, C = training_pair(who, XTX, XTY)
    check_dims(K, C, A, limit)
    cw = check_class_weights(class_weights, F, C, XTX.device)
    pca = pcr_fit_batched(XTX, None, A, return_components=True, solver=solver, rank_tol=rank_tol,
                          max_sweeps=max_sweeps)
    return pcalda_from_components(pca.components, pca.eigenvalues, pca.n_fit, XTY, cw, pivot_tol=pivot_tol,
                                  check=check)


def cv_pcalda(cvm, folds, A, **kw):
    """Fold stage, class weights and ``pcalda_fit_batched`` in one call: ``(fit, stats)``, ``stats`` being the
    statistics tuple ``lda_cv_decision`` and ``lda_cv_predict`` take.  ``cv_lda``'s counterpart, and like it the
    one place the model's flags are checked: raises ``ValueError`` unless ``center_X`` is set and ``scale_Y`` is
    not.  ``kw``: the keywords of ``pcalda_fit_batched``."""
    if not cvm.center_X:
        raise ValueError("cv_pcalda needs a CVMatrix with center_X=True: the class sums must be sums of centred rows.")
    if cvm.scale_Y:
        raise ValueError("cv_pcalda needs a CVMatrix with scale_Y=False: Y is the 0/1 class indicator.")
    check_components(A)
    check_pivot_tol(kw.get("pivot_tol"))
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    fit = pcalda_fit_batched(XTX, XTY, training_class_weights(cvm, batch), A, **kw)
    return fit, stats
