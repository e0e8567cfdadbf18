"""
CPU oracle for the step AFTER the cvmatrix hot path: an
Improved-Kernel-PLS fit on the training matrices ``(XTX_T, XTY_T)`` of one fold --
TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only ``tests/``, ``__graft_entry__.smoke()`` and
``bench.py``'s CPU leg may import it; nothing under ``cvmatrix_amd/`` does.

What it restates.  The consumer the reference names is the out-of-tree package ``ikpls``
(reference README.md:23, cvmatrix/partitioner.py:27-31): its fast cross-validation runs
"Improved Kernel PLS Algorithm #2" of Dayal & MacGregor, *Improved PLS algorithms*,
J. Chemometrics 11 (1997) 73-85, on each fold's ``XTX``/``XTY``.  ``ikpls`` is NOT present in
/root/reference (no vendored copy, no pinned version: the reference only links to it) and not
installed in the image, so this is a restatement of the PUBLISHED algorithm:

    for a = 1..A:
        w   = dominant left singular vector of XTY           (M == 1: XTY / |XTY|;
              M > 1: XTY q / |XTY q| with q the eigenvector of the largest eigenvalue of XTY^T XTY)
        r   = w - sum_{j<a} (p_j^T w) r_j
        tTt = r^T XTX r
        p   = XTX r / tTt                                    (XTX is symmetric)
        q   = XTY^T r / tTt
        XTY = XTY - (p q^T) tTt
        B_a = B_{a-1} + r q^T

Parity status: PINNED AGAINST scikit-learn, UNPINNED AGAINST ikpls ITSELF.  PLS2 by NIPALS
(``sklearn.cross_decomposition.PLSRegression``, scale=False, converged inner loop) defines the
same model: tests/test_pls_oracle.py checks the regression coefficients of this restatement
against scikit-learn 1.7.2 live and against ``tests/golden/g8_pls.npz`` (made by
``tests/golden/make_golden_pls.py``).  The sign of each component (w, p, q, r) is not
defined by the algorithm (an eigenvector's sign is arbitrary); ``B`` does not depend on it.

Stopping rule: when |XTY q| is not above ``eps`` of the dtype the remaining components cannot
be extracted; the loop stops, ``n_fit`` says how many were, and the arrays keep zeros beyond.
"""

from __future__ import annotations

import numpy as np


def dominant_q_squaring(S: np.ndarray) -> np.ndarray:
    """The dominant eigenvector of the symmetric positive semi-definite ``S`` the way the device
    kernel says it finds it (``pls_dominant_q``, cvmatrix_amd/csrc/pls.hpp), restated in float64 NumPy:
    ``m = S / trace``; ``m <- m^2 / sum(m^2)`` (``sum(m^2)`` of the symmetric trace-1 input is
    ``sum lambda^2``) until ``1 - sum(m^2) < 1e-13`` or 64 squarings; the column of the largest diagonal
    entry, the lowest index among equals; two power steps with ``S`` itself, each normalised.  A trace
    that is not positive gives the zero vector.  It is a statement of the method, not of the kernel's
    summation orders: its Rayleigh quotient is the yardstick for the kernel's, its bits are not."""
    S = np.asarray(S, dtype=np.float64)
    M = S.shape[0]
    tr = float(np.trace(S))
    if not tr > 0.0:
        return np.zeros(M)
    m = S / tr
    for _ in range(64):
        t2 = float(np.sum(m * m))
        m = (m @ m) / t2
        if 1.0 - t2 < 1e-13:
            break
    q = m[:, int(np.argmax(np.maximum(np.diag(m), 0.0)))].copy()       # argmax: the first among equals
    for _ in range(2):
        v = S @ q
        nn = float(np.sqrt(v @ v))
        q = v / nn if nn > 0.0 else np.zeros(M)
    return q


def ikpls_follow(XTX: np.ndarray, XTY: np.ndarray, W: np.ndarray, dtype=np.longdouble):
    """The published algorithm with the weight vector of component ``a`` GIVEN (``W[:, a]``, taken as it
    is: neither recomputed nor normalised) and everything else computed in ``dtype``: given the same
    weights, r, u = XTX r, tTt, p, q, the deflation and B are determined, so a fit can be compared
    with a reference that does not have to find an eigenvector.  Plain loops and ``@``.

    Returns ``(B, P, Q, R, tTt, Ys)``: ``B`` (A,K,M); ``P, R`` (K,A); ``Q`` (M,A); ``tTt`` (A,);
    ``Ys`` (A,K,M), the deflated XTY BEFORE each component.  With ``dtype=np.float64`` the operations
    and their order are those of ``ikpls_fit`` (the same bits from the same weights)."""
    dt = np.dtype(dtype)
    if dt == np.longdouble:
        assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the x86 80-bit format here"
    XTX = np.asarray(XTX).astype(dt)
    Y = np.array(XTY, dtype=dt, copy=True)
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)
    W = np.asarray(W).astype(dt)
    K, M = Y.shape
    A = W.shape[1]
    B = np.zeros((A, K, M), dt)
    P = np.zeros((K, A), dt)
    Q = np.zeros((M, A), dt)
    R = np.zeros((K, A), dt)
    tTt = np.zeros(A, dt)
    Ys = np.zeros((A, K, M), dt)
    for a in range(A):
        Ys[a] = Y
        w = W[:, a]
        r = w.copy()
        if a:
            r -= R[:, :a] @ (P[:, :a].T @ w)
        u = XTX @ r
        t = r @ u
        p = u / t
        q = (Y.T @ r) / t
        Y -= np.outer(p, q) * t
        P[:, a], Q[:, a], R[:, a], tTt[a] = p, q, r, t
        B[a] = (B[a - 1] if a else 0) + np.outer(r, q)
    return B, P, Q, R, tTt, Ys


def ikpls_fit(XTX: np.ndarray, XTY: np.ndarray, A: int, eig: str = "eigh"):
    """Returns ``(B, W, P, Q, R, n_fit)`` with ``B`` (A,K,M); ``W, P, R`` (K,A); ``Q`` (M,A).

    ``B[a]`` are the regression coefficients of the model with ``a + 1`` components, for
    centred/scaled predictors and responses exactly as ``XTX``/``XTY`` were.  ``eig``: where the
    eigenvector of XTY^T XTY comes from for M > 1 -- "eigh" (LAPACK) or "squaring"
    (``dominant_q_squaring``, the device kernel's method).
    """
    if eig not in ("eigh", "squaring"):
        raise ValueError("eig must be 'eigh' or 'squaring'")
    XTX = np.asarray(XTX)
    dtype = XTX.dtype
    XTY = np.array(XTY, dtype=dtype, copy=True)
    if XTY.ndim == 1:
        XTY = XTY.reshape(-1, 1)
    K, M = XTY.shape
    B = np.zeros((A, K, M), dtype)
    W = np.zeros((K, A), dtype)
    P = np.zeros((K, A), dtype)
    Q = np.zeros((M, A), dtype)
    R = np.zeros((K, A), dtype)
    eps = np.finfo(dtype).eps
    n_fit = 0
    for a in range(A):
        if M == 1:
            w = XTY[:, 0].copy()
        else:
            S = XTY.T @ XTY
            if eig == "squaring":
                w = XTY @ dominant_q_squaring(S)
            else:
                _, vecs = np.linalg.eigh(S)
                w = XTY @ vecs[:, -1]
        nrm = np.sqrt(w @ w)
        if not nrm > eps:
            break
        w = w / nrm
        r = w.copy()
        if a:
            r -= R[:, :a] @ (P[:, :a].T @ w)
        u = XTX @ r
        tTt = r @ u
        p = u / tTt
        q = (XTY.T @ r) / tTt
        XTY -= np.outer(p, q) * tTt
        W[:, a], P[:, a], Q[:, a], R[:, a] = w, p, q, r
        B[a] = (B[a - 1] if a else 0) + np.outer(r, q)
        n_fit = a + 1
    return B, W, P, Q, R, n_fit


def predict(B: np.ndarray, Xs: np.ndarray) -> np.ndarray:
    """``Xs`` (n,K) already centred/scaled like the training data -> (A,n,M) predictions in the
    centred/scaled response space, one per number of components."""
    return np.einsum("nk,akm->anm", Xs, B)
