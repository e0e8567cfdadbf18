"""Reference for the device ridge (cvm_ridge_fit): NumPy only, never imported by the product.

``ridge_solve_ref`` solves ``(XTX + lam I) B = XTY`` to well beyond float64: a float64 Cholesky solve
followed by iterative refinement on a residual that is formed without rounding error to speak of.

The residual.  ``np.longdouble`` alone (64-bit significand on x86) is not enough: a residual rounded at
2^-64 of ``|A| |B|`` leaves an error of ``cond(A) * 2^-64`` in the refined solution -- 5e-8 at
cond 1e12, and no correction ever falls below 1e-18.  So the products are made exact instead.  B is kept
as an unevaluated sum of two float64 arrays; every row of XTX and every column of B is cut on a fixed
binary grid into slices of ``beta`` bits, with ``2 beta + 1 + log2 K <= 53`` so that the float64 matrix
product of two slices is exact whatever order the BLAS sums in (every partial sum is an integer of at
most 53 bits times a power of two; Ozaki, Ogita, Oishi, Rump 2012); the slice products that matter
(126 bits below ``max|row| * max|column|``) and ``lam B`` (lam cut the same way) are summed with an
error-free two-sum whose error terms are accumulated in float64, i.e. in twice the working precision.
The residual then carries an error near ``2^-105 |A| |B|``, the refined solution ``cond * 2^-105``:
1e-20 at cond 1e12.  The matrix is ``XTX + lam I`` with the diagonal NOT rounded.

``np.longdouble`` is used for what it is good for: the norm of the correction and of B in the
convergence check, which must resolve 1e-18.  The module checks ``np.finfo(np.longdouble).eps <= 2**-63``
(``LONGDOUBLE_OK``); where that does not hold ``ridge_solve_ref`` raises ``RuntimeError`` and the tests
that need it skip with ``LONGDOUBLE_REASON``."""

from __future__ import annotations

import numpy as np

U = 2.0 ** -53                                   # unit roundoff of float64
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
LONGDOUBLE_REASON = f"np.longdouble has eps {np.finfo(np.longdouble).eps!r} > 2**-63 on this platform"

CONVERGED = 1e-18                                # relative size of the last correction
MAX_ROUNDS = 10
N_SLICES = 6


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _grid_exponent(X, axis):
    """e with max|X| along `axis` < 2**e (keepdims); 0 where the maximum is 0."""
    mx = np.max(np.abs(X), axis=axis, keepdims=True)
    _, e = np.frexp(mx)
    return np.where(mx > 0, e, 0)


def _slices(parts, e, beta, n):
    """Cut the unevaluated sum of the float64 arrays `parts` on the grid 2**(e - k beta), k = 1..n:
    slice k is a multiple of 2**(e - k beta) of magnitude at most (len(parts) * 2**(beta - 1) + 1) grid
    steps (2**beta for k = 1).  What lies below the last grid step is dropped."""
    rem = [np.array(p, dtype=np.float64) for p in parts]
    out = []
    for k in range(1, n + 1):
        sigma = np.ldexp(1.5, 52 + e - k * beta)     # x + sigma has its last bit at 2**(e - k beta)
        sl = 0.0
        for i, r in enumerate(rem):
            hi = (r + sigma) - sigma
            rem[i] = r - hi                          # exact
            sl = sl + hi                             # exact: both on the grid, a few bits wide
        out.append(sl)
    return out


def _residual(XTX, XTY, lam, Bh, Bl):
    """XTY - (XTX + lam I)(Bh + Bl), rounded once to float64 from a sum carried in twice the precision."""
    K = XTX.shape[0]
    beta = (52 - int(np.ceil(np.log2(max(K, 2))))) // 2
    n = N_SLICES
    As = _slices([XTX], _grid_exponent(XTX, 1), beta, n)
    Bs = _slices([Bh, Bl], _grid_exponent(Bh, 0), beta, n)
    _, el = np.frexp(lam)
    Ls = _slices([np.float64(lam)], int(el), beta, 3) if lam != 0.0 else []
    hi = np.array(XTY, dtype=np.float64)
    lo = np.zeros_like(hi)
    terms = []
    for i in range(n):
        for j in range(n - i):
            terms.append((i + j, As[i] @ Bs[j]))     # exact
    for i, l in enumerate(Ls):
        for j in range(n):
            terms.append((i + j, l * Bs[j]))         # exact: (beta + 1) + beta bits
    terms.sort(key=lambda t: t[0])
    for _, t in terms:
        hi, err = _two_sum(hi, -t)
        lo += err
    return hi + lo


def _cho_solve(Lc, R):
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, R))


def ridge_solve_ref(XTX, XTY, lam):
    """The solution of ``(XTX + lam I) B = XTY``, float64 (K, M), for practical purposes correctly
    rounded.  Raises ``np.linalg.LinAlgError`` where the float64 Cholesky fails or the refinement has not
    converged to 1e-18 in 10 rounds: such a case is too ill-conditioned to be a fixture."""
    if not LONGDOUBLE_OK:
        raise RuntimeError(LONGDOUBLE_REASON)
    XTX = np.array(XTX, dtype=np.float64)
    XTY = np.array(XTY, dtype=np.float64)
    one_col = XTY.ndim == 1
    if one_col:
        XTY = XTY[:, None]
    lam = float(lam)
    K = XTX.shape[0]
    if not (np.all(np.isfinite(XTX)) and np.all(np.isfinite(XTY))):
        raise np.linalg.LinAlgError("ridge_solve_ref: input is not finite")
    Lc = np.linalg.cholesky(XTX + lam * np.eye(K))
    Bh = _cho_solve(Lc, XTY)
    Bl = np.zeros_like(Bh)
    for _ in range(MAX_ROUNDS):
        d = _cho_solve(Lc, _residual(XTX, XTY, lam, Bh, Bl))
        s, err = _two_sum(Bh, d)
        Bl = Bl + err
        Bh = s + Bl                                  # renormalise (fast two-sum: |Bl| << |s|)
        Bl = Bl - (Bh - s)
        nd = np.sqrt(np.sum(d.astype(np.longdouble) ** 2))
        nb = np.sqrt(np.sum(Bh.astype(np.longdouble) ** 2))
        if nd <= np.longdouble(CONVERGED) * nb:
            return Bh[:, 0] if one_col else Bh
    raise np.linalg.LinAlgError(f"ridge_solve_ref: no convergence in {MAX_ROUNDS} rounds (last correction "
                                f"{float(nd / nb) if nb else float('nan'):.2e} relative)")


def cholesky_pivots(A):
    """A plain unblocked float64 Cholesky (column by column, inner products by ``@``): ``(info, pivots)``
    with info = 0 and all K pivots (the squares of the diagonal of L), or info = the 1-based index of the
    first pivot that is not finite or not > 0 and the pivots up to and including that one."""
    A = np.array(A, dtype=np.float64)
    K = A.shape[0]
    Lc = np.zeros((K, K))
    piv = np.empty(K)
    with np.errstate(all="ignore"):
        for j in range(K):
            p = A[j, j] - Lc[j, :j] @ Lc[j, :j]
            piv[j] = p
            if not (np.isfinite(p) and p > 0):
                return j + 1, piv[:j + 1]
            d = np.sqrt(p)
            Lc[j, j] = d
            Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / d
    return 0, piv


def cholesky_info(A):
    """``(info, pivot)``: 0 and the smallest pivot, or the 1-based index of the first pivot that is not
    finite or not > 0 (as LAPACK potrf counts) and the value of that pivot."""
    info, piv = cholesky_pivots(A)
    return (info, float(piv[-1])) if info else (0, float(piv.min()))


def rel_err(B, ref):
    """Relative Frobenius error."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(B, dtype=np.float64) - ref) / np.linalg.norm(ref))


def yardstick(XTX, XTY, lam, ref=None):
    """The larger relative Frobenius forward error, against ``ridge_solve_ref``, of the two float64 solves
    NumPy offers: ``np.linalg.solve`` and ``np.linalg.cholesky`` with two triangular solves."""
    XTX = np.asarray(XTX, dtype=np.float64)
    XTY = np.asarray(XTY, dtype=np.float64)
    if ref is None:
        ref = ridge_solve_ref(XTX, XTY, lam)
    A = XTX + float(lam) * np.eye(XTX.shape[0])
    return max(rel_err(np.linalg.solve(A, XTY), ref), rel_err(_cho_solve(np.linalg.cholesky(A), XTY), ref))
