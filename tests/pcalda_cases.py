"""Designs, the reference and the accuracy gate of the device PCA-LDA tests (tests/test_gpu_pcalda.py on the GPU;
tests/test_pcalda_host.py checks on the CPU that the reference is scikit-learn's Pipeline(PCA, LDA(lsqr)) and that
every design meets its own conditions).  NumPy and the oracle only: nothing here touches the product.

Inputs.  The rows come from tests/lda_cases.py; the eigenpairs are ``numpy.linalg.eigh`` of the fold's XTX, so
that the device (``pcalda_from_components``) and the yardstick see the same bits of V, eig, XTY and class_w.

Truth.  From those very bits, in ``np.longdouble``, for every number of components a on its own (no running
sum): P = V^T H, S_a = diag(lambda_a) - sum_c p_c p_c^T / n_c, M~_a = P_a / n_c; ``S_a x = M~_a`` by
``oracle.ridge_oracle.ridge_solve_ref`` at lambda = 0 -- on S_a rounded to float64, followed by one correction
with the parts of S_a and M~_a that the rounding dropped, which leaves cond(S_a)^2 u^2; then n V_a x and
-1/2 n m~_c . x_c + log(n_c / n) in longdouble.

Yardstick.  The same route in plain NumPy float64 (``np.linalg.solve`` per a); Y is its relative error against
the truth, the largest over the folds of the batch.

Gate.  ``err <= 2 Y + c u`` (float32: + 2^-24 for the store).  err: the relative Frobenius error of coef[f, a] over
the present classes; for intercept[f, a] the largest error over the largest finite magnitude.  c counts the
roundings of the kernels' order of operations (cvmatrix_amd/csrc/pcalda.hpp) that Y does not stand for; it is
derived here and never calibrated on the device:
  * the projections: p = sum_k v_k h_k is one fma per row within a slice of 128 rows and one addition per slice,
    K + ceil(K / 128) roundings, each relative to |v| . |h| while the result has the size of p: times
    rho = || |V_a|^T |H| ||_F / ||P_a||_F of the fixture;
  * the downdate: an entry of S is lambda_j [i = j] - sum_c (p_c[i] (1 / n_c)) p_c[j]: per class the reciprocal,
    the product and the fma, and the pivot's subtraction and square root: 3 C + 2 roundings, each relative to a
    term of the size of lambda_j while the result has the size of S: times amp = ||diag lambda_a||_F / ||S_a||_F,
    the largest over a and the folds;
  * the substitutions: m~ = p / n_c (1), row j of Z = L^-1 M~ (j fma and a division), row j of X = L^-1 (likewise),
    row k of W = V X^T (j + 1 fma): at most 3 (a + 1) + 3 for the model on a + 1 components;
  * the running sum: n z (1) and one fma per component, a + 1; the intercept likewise, with the two roundings of
    log(n_c / n) in place of the product's.
  c(a) = (K + ceil(K / 128)) rho + (3 C + 2) amp + 4 (a + 1) + 6.

Pivots.  ``reference_path`` runs the factorisation with the stopping rule in longdouble and returns the pivots;
the decisions (n_fit, info) are compared exactly, which is fair where every accepted pivot is >= 100 pivot_tol
lambda_j and every rejected one <= pivot_tol lambda_j / 100 in magnitude (tests/test_pcalda_host.py)."""

import functools
import os

import numpy as np

import lda_cases as lc
from oracle import ridge_oracle as ro

U = ro.U
LD = np.longdouble
PIVOT_TOL = 2.0 ** -26
KSLICE = 128                      # PCL_KSLICE of cvmatrix_amd/csrc/pcalda.hpp
N_FOLDS = 3

K_VALUES = (1, 2, 31, 32, 33, 64, 65, KSLICE + 1, 257)
C_VALUES = (2, 3, 17, 64)
# (K, C, A): every K, every C, A in {1, 2, min(K, 5), min(K, 64)}; both sides of the 32-row tile, of the 64-component
# cap and of the 128-row slice
GRID = [(1, 2, 1), (1, 64, 1), (2, 3, 2), (2, 17, 1), (31, 2, 31), (31, 64, 5), (32, 17, 32), (32, 3, 2), (33, 3, 33),
        (33, 64, 5), (64, 2, 64), (64, 64, 64), (65, 17, 64), (65, 3, 5), (KSLICE + 1, 3, 64), (KSLICE + 1, 17, 5),
        (257, 2, 64), (257, 17, 5), (257, 64, 64)]
GRID_F32 = [(2, 3, 2), (33, 64, 5), (64, 64, 64), (65, 17, 64), (KSLICE + 1, 3, 64), (257, 17, 5)]

LADDER_KCA = (33, 3, 12)
LADDER_SEP = lc.LADDER_SEP
# at 1e4 standard deviations between the classes the within-class share of the leading components' variance is
# 1e-8: the default pivot_tol sits there on purpose, so the ladder (a test of the cancellation, not of the stopping
# rule) runs with a threshold that every pivot clears by 100 and more
LADDER_PIVOT_TOL = 2.0 ** -40


# ---- inputs: what the device is handed

def default_rank_tol(K):
    return 32.0 * K * 2.0 ** -52


def eig_inputs(XTX, A):
    """(V (F,K,A), eig (F,A) descending, n_comp (F,) int32) of a batch by ``numpy.linalg.eigh``: n_comp counts the
    eigenvalues above 32 K 2^-52 times the largest, at most A (the rule of the device's eigensolvers)."""
    XTX = np.asarray(XTX, dtype=np.float64)
    F, K, _ = XTX.shape
    V, E, nc = np.empty((F, K, A)), np.empty((F, A)), np.empty(F, dtype=np.int32)
    for f in range(F):
        lam, Q = np.linalg.eigh(XTX[f])
        lam, Q = lam[::-1], Q[:, ::-1]
        V[f], E[f] = Q[:, :A], lam[:A]
        nc[f] = min(A, int(np.sum(lam > default_rank_tol(K) * lam[0])))
    return V, E, nc


def batch_inputs(X, y, w, folds, C, A, dtype=np.float64, scale=False):
    """(V, eig, n_comp, XTY, class weights) of a list of validation index arrays; V and XTY in ``dtype``."""
    XTX, XTY, CW = lc.batch_inputs(X, y, w, folds, C, scale=scale)
    V, E, nc = eig_inputs(XTX, A)
    return V.astype(dtype), E, nc, XTY.astype(dtype), CW


@functools.lru_cache(maxsize=None)
def grid_case(K, C, A):
    X, y, w = lc.grid_rows(K, C)
    return batch_inputs(X, y, w, lc.folds_of(X.shape[0], C), C, A)


@functools.lru_cache(maxsize=None)
def ladder_case(sep):
    K, C, A = LADDER_KCA
    X, y, w = lc.ladder_rows(sep)
    return batch_inputs(X, y, w, lc.folds_of(X.shape[0], C), C, A)


# ---- the path: pivots and decisions

def scatter_ld(V, eig, XTY, cw):
    """(P (A,C), S (A,A), M~ (A,C)) in longdouble from the bits handed to the device."""
    V, H = np.asarray(V, dtype=np.float64).astype(LD), np.asarray(XTY, dtype=np.float64).astype(LD)
    cwl = np.asarray(cw, dtype=np.float64).astype(LD)
    P = V.T @ H
    present = cwl > 0
    Mt = np.zeros_like(P)
    Mt[:, present] = P[:, present] / cwl[present]
    S = np.diag(np.asarray(eig, dtype=np.float64).astype(LD)) - Mt @ P.T
    return P, 0.5 * (S + S.T), Mt


def reference_path(V, eig, n_comp, XTY, cw, pivot_tol=PIVOT_TOL):
    """(n_fit, info, pivots): the column-by-column factorisation of S with the stopping rule, in longdouble.
    ``pivots`` holds d_j^2 of every accepted component and, where the path ended at a pivot, the rejected one."""
    A = len(eig)
    _, S, _ = scatter_ld(V, eig, XTY, cw)
    L = np.zeros((A, A), dtype=LD)
    piv = []
    for j in range(A):
        if j >= n_comp:
            return j, 1, np.array(piv, dtype=np.float64)
        d2 = S[j, j] - L[j, :j] @ L[j, :j]
        piv.append(float(d2))
        if not d2 > LD(pivot_tol) * LD(eig[j]):
            return j, 2, np.array(piv, dtype=np.float64)
        d = np.sqrt(d2)
        L[j, j] = d
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / d
    return A, 0, np.array(piv, dtype=np.float64)


def pivot_margins(V, eig, n_comp, XTY, cw, pivot_tol=PIVOT_TOL):
    """(the smallest accepted pivot over pivot_tol lambda_j, the rejected pivot's magnitude over pivot_tol
    lambda_j or 0.0 where none was rejected)."""
    n_fit, info, piv = reference_path(V, eig, n_comp, XTY, cw, pivot_tol)
    thr = pivot_tol * np.asarray(eig, dtype=np.float64)
    acc = min((piv[j] / thr[j] for j in range(n_fit)), default=np.inf)
    rej = abs(piv[n_fit]) / thr[n_fit] if info == 2 else 0.0
    return acc, rej


# ---- the truth and the yardstick

def _solve_ld(S, Mt):
    """S x = M~ for longdouble S, M~: the oracle on the float64 roundings, then one correction with what the
    roundings dropped.  Returns x in longdouble."""
    Sh, Mh = S.astype(np.float64), Mt.astype(np.float64)
    Sl, Ml = S - Sh.astype(LD), Mt - Mh.astype(LD)
    x0 = ro.ridge_solve_ref(Sh, Mh, 0.0)
    r = (Ml - Sl @ x0.astype(LD)).astype(np.float64)
    x1 = ro.ridge_solve_ref(Sh, r, 0.0) if np.any(r) else np.zeros_like(x0)
    return x0.astype(LD) + x1.astype(LD)


def truth_fold(V, eig, XTY, cw, n_models):
    """coef (n_models,K,C), intercept (n_models,C) float64 of one fold, every a on its own.  An absent class has
    coef 0 and intercept -inf."""
    P, S, Mt = scatter_ld(V, eig, XTY, cw)
    Vl = np.asarray(V, dtype=np.float64).astype(LD)
    cwl = np.asarray(cw, dtype=np.float64).astype(LD)
    n = cwl.sum()
    K, C = Vl.shape[0], P.shape[1]
    present = np.asarray(cw) > 0
    coef = np.zeros((n_models, K, C))
    icpt = np.full((n_models, C), -np.inf)
    for a in range(n_models):
        x = _solve_ld(S[:a + 1, :a + 1], Mt[:a + 1])
        coef[a] = (n * (Vl[:, :a + 1] @ x)).astype(np.float64)
        coef[a][:, ~present] = 0.0
        ic = -0.5 * n * np.sum(Mt[:a + 1] * x, axis=0)[present] + np.log(cwl[present] / n)
        icpt[a, present] = ic.astype(np.float64)
    return coef, icpt


def restate_fold(V, eig, XTY, cw, n_models):
    """The same route in NumPy float64."""
    V, H, cw = (np.asarray(t, dtype=np.float64) for t in (V, XTY, cw))
    n = cw.sum()
    present = cw > 0
    P = V.T @ H
    Mt = np.zeros_like(P)
    Mt[:, present] = P[:, present] / cw[present]
    S = np.diag(np.asarray(eig, dtype=np.float64)) - Mt @ P.T
    K, C = H.shape
    coef = np.zeros((n_models, K, C))
    icpt = np.full((n_models, C), -np.inf)
    for a in range(n_models):
        x = np.linalg.solve(S[:a + 1, :a + 1], Mt[:a + 1])
        coef[a] = n * (V[:, :a + 1] @ x)
        coef[a][:, ~present] = 0.0
        icpt[a, present] = (-0.5 * n * np.sum(Mt[:a + 1] * x, axis=0) + np.log(np.where(present, cw, 1.0) / n))[present]
    return coef, icpt


def prior_only(cw, K):
    """The model on no component: coef 0, intercept the log priors (-inf for an absent class)."""
    cw = np.asarray(cw, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.zeros((K, cw.size)), np.log(cw / cw.sum())


def rho_amp(V, eig, XTY, cw, n_models):
    """(rho, amp) of one fold: the cancellation factors of the projections and of the downdate, the largest over
    a < n_models."""
    V, H = np.asarray(V, dtype=np.float64), np.asarray(XTY, dtype=np.float64)
    _, S, _ = scatter_ld(V, eig, XTY, cw)
    S = S.astype(np.float64)
    absP, P = np.abs(V).T @ np.abs(H), V.T @ H
    rho = amp = 1.0
    for a in range(n_models):
        rho = max(rho, np.linalg.norm(absP[:a + 1]) / np.linalg.norm(P[:a + 1]))
        amp = max(amp, np.linalg.norm(np.asarray(eig[:a + 1], dtype=np.float64)) / np.linalg.norm(S[:a + 1, :a + 1]))
    return rho, amp


def gate_c(K, C, a, rho, amp):
    return (K + -(-K // KSLICE)) * rho + (3 * C + 2) * amp + 4 * (a + 1) + 6


def coef_err(coef, ref, present):
    return ro.rel_err(np.asarray(coef, dtype=np.float64)[:, present], ref[:, present])


def icpt_err(icpt, ref, present):
    icpt, ref = np.asarray(icpt, dtype=np.float64)[present], ref[present]
    return float(np.abs(icpt - ref).max() / np.abs(ref).max())


class Reference:
    """Truth, yardsticks and the gate's constants of a batch, for the models a < n_fit[f] of every fold (the
    reference path's n_fit): computed once, shared, never changed."""

    def __init__(self, V, eig, n_comp, XTY, CW, pivot_tol=PIVOT_TOL):
        F, K, A = V.shape
        C = XTY.shape[2]
        self.F, self.K, self.A, self.C = F, K, A, C
        self.n_fit, self.info = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        self.coef, self.icpt = np.zeros((F, A, K, C)), np.zeros((F, A, C))
        self.Yc, self.Yi = np.zeros(A), np.zeros(A)
        self.rho = self.amp = 1.0
        self.present = np.asarray(CW) > 0
        for f in range(F):
            nf, info, _ = reference_path(V[f], eig[f], n_comp[f], XTY[f], CW[f], pivot_tol)
            self.n_fit[f], self.info[f] = nf, info
            coef, icpt = truth_fold(V[f], eig[f], XTY[f], CW[f], nf)
            mine_c, mine_i = restate_fold(V[f], eig[f], XTY[f], CW[f], nf)
            pr = self.present[f]
            for a in range(nf):
                self.Yc[a] = max(self.Yc[a], coef_err(mine_c[a], coef[a], pr))
                self.Yi[a] = max(self.Yi[a], icpt_err(mine_i[a], icpt[a], pr))
            if nf:
                rho, amp = rho_amp(V[f], eig[f], XTY[f], CW[f], nf)
                self.rho, self.amp = max(self.rho, rho), max(self.amp, amp)
            # the padding: the last model that exists, or the prior-only model
            last = (coef[nf - 1], icpt[nf - 1]) if nf else prior_only(CW[f], K)
            self.coef[f, :nf], self.icpt[f, :nf] = coef, icpt
            self.coef[f, nf:], self.icpt[f, nf:] = last

    def bounds(self, a, float32=False):
        c = gate_c(self.K, self.C, a, self.rho, self.amp)
        store = 2.0 ** -24 if float32 else 0.0
        return store + 2.0 * self.Yc[a] + c * U, store + 2.0 * self.Yi[a] + c * U


@functools.lru_cache(maxsize=None)
def grid_reference(K, C, A):
    return Reference(*grid_case(K, C, A))


def assert_gate(coef, icpt, ref, what, float32=False):
    """Every model that exists, of every fold, against the gate; returns the largest err / Y.
    CVM_PCALDA_REPORT=path: one line per comparison."""
    coef, icpt = np.asarray(coef, dtype=np.float64), np.asarray(icpt, dtype=np.float64)
    report = os.environ.get("CVM_PCALDA_REPORT")
    lines, bad, worst = [], [], 0.0
    for f in range(ref.F):
        pr = ref.present[f]
        for a in range(ref.n_fit[f]):
            ec, ei = coef_err(coef[f, a], ref.coef[f, a], pr), icpt_err(icpt[f, a], ref.icpt[f, a], pr)
            bc, bi = ref.bounds(a, float32)
            worst = max(worst, ec / ref.Yc[a] if ref.Yc[a] > 0 else 0.0, ei / ref.Yi[a] if ref.Yi[a] > 0 else 0.0)
            lines.append(f"{what} f={f} a={a}\tcoef {ec:.3e} Y {ref.Yc[a]:.3e} bound {bc:.3e}\t"
                         f"intercept {ei:.3e} Y {ref.Yi[a]:.3e} bound {bi:.3e}\n")
            if not (ec <= bc and ei <= bi):
                bad.append(lines[-1].strip())
    if report:
        with open(report, "a") as fh:
            fh.writelines(lines)
    assert not bad, f"{what}: error above 2 Y + c u" + (" + 2^-24" if float32 else "") + ": " + "; ".join(bad[:6])
    return worst


# ---- the stopping designs

def stopping_pivot_case():
    """tests/lda_cases.singular_case with A = 32: fold 1 trains on 30 rows of K = 40 in C = 3 classes, so its
    scatter has rank 27: the path ends at the 28th pivot (n_fit 27, info 2); the other folds have all 32 models."""
    X, y, folds, C = lc.singular_case()
    return batch_inputs(X, y, None, folds, C, 32)


def stopping_rank_case():
    """K = 24, C = 3, A = 16 on rows that span 10 dimensions only (120 training rows a fold): n_comp = 10 < A and
    every pivot is sound, so the path ends at the components that exist (n_fit 10, info 1)."""
    K, C, N, A, R = 24, 3, 180, 16, 10
    rng = np.random.default_rng(24)
    X, y, _ = lc.make_rows(24, N, R, C)
    B = np.linalg.qr(rng.standard_normal((K, R)))[0]               # the rows live in a 10-dimensional subspace
    X = X @ B.T
    return batch_inputs(X, y, None, lc.folds_of(N, C), C, A)


def separated_case():
    """Two classes that differ along the first component only and have no variance there: x_0 = -1 in class 0 and
    +2 in class 1 (centred: the class means carry all of that direction's variance), small noise in the other
    K - 1 variables.  The first pivot is lambda_0 - sum_c p_c^2 / n_c = 0 up to rounding: n_fit 0, info 2, the
    prior-only model.  One fold (fold 1 of 3) is like that; the others are ordinary grid folds."""
    K, C, A = 6, 2, 4
    V, E, nc, XTY, CW = (t.copy() for t in grid_case_small(K, C, A))
    rng = np.random.default_rng(6)
    N = 40
    y = (np.arange(N) % 3 == 0).astype(int)                          # 14 rows of class 1, 26 of class 0
    X = 1e-3 * rng.standard_normal((N, K))
    X[:, 0] = np.where(y == 1, 2.0, -1.0)
    X -= X.mean(axis=0)
    Y = lc.indicator(y, C)
    XTX = X.T @ X
    v, e, n1 = eig_inputs(0.5 * (XTX + XTX.T)[None], A)
    V[1], E[1], nc[1], XTY[1], CW[1] = v[0], e[0], n1[0], X.T @ Y, Y.sum(axis=0)
    return V, E, nc, XTY, CW


def grid_case_small(K, C, A):
    X, y, w = lc.make_rows(1000 * K + C, 6 * (K + C) + 45, K, C)
    return batch_inputs(X, y, w, lc.folds_of(X.shape[0], C), C, A)


def absent_case(A=12):
    """tests/lda_cases.absent_case (K = 33, C = 4: fold 1 trains without class 2) with A components."""
    X, y, folds, C = lc.absent_case()
    return batch_inputs(X, y, None, folds, C, A)


# ---- end to end

E2E = dict(N=600, K=12, C=4, F=5, A=8)
E2E_SKIP_CAP = 0.01
E2E_DECAY = 0.75


def e2e_rows(weighted):
    """600 rows of 12 correlated variables in 4 classes: latent variables with standard deviations 0.75^k and class
    means of that size, mixed by a random orthogonal matrix (so that the spectrum of the training scatter decays
    with or without scaling and the leading subspaces are determined), an offset so that centring matters;
    5 folds and rows in no fold, dealt as tests/lda_cases.e2e_rows deals them."""
    N, K, C, F = E2E["N"], E2E["K"], E2E["C"], E2E["F"]
    rng = np.random.default_rng(1600 + int(weighted))
    y = (np.arange(N) % (C + 1)) % C
    s = E2E_DECAY ** np.arange(K)
    Q = np.linalg.qr(rng.standard_normal((K, K)))[0]
    means = 1.5 * rng.standard_normal((C, K)) * s
    X = (rng.standard_normal((N, K)) * s + means[y]) @ Q + 0.5
    w = rng.integers(1, 4, N).astype(np.float64) if weighted else None
    labels = (np.arange(N) // (C + 1)) % (F + 1)                     # label F: rows in no fold
    folds = [np.flatnonzero(labels == f) for f in range(F)]
    return X, y, w, folds, np.flatnonzero(labels == F)


def row_reference_fold(X, y, w, val, C, A, scale=False):
    """The row-based reference of one fold: PCA by the SVD of the standardised training rows (replicated by their
    integer weights), lsqr LDA on the scores of the first a + 1 components for every a.  Returns (coef (A,K,C),
    intercept (A,C)) for standardised rows, the singular values squared (K,), and the training statistics."""
    tr, wt, mu, sd = lc.training_stats(X, w, val, scale)
    rep = np.repeat(np.arange(tr.size), wt.astype(int))
    Z = ((X[tr] - mu) / sd)[rep]
    yt = y[tr][rep]
    n = Z.shape[0]
    _, sv, Vt = np.linalg.svd(Z, full_matrices=False)
    K = Z.shape[1]
    coef = np.zeros((A, K, C))
    icpt = np.full((A, C), -np.inf)
    for a in range(A):
        Va = Vt[:a + 1].T
        T = Z @ Va
        means = np.stack([T[yt == c].mean(axis=0) for c in range(C)])
        Sw = sum((T[yt == c] - means[c]).T @ (T[yt == c] - means[c]) for c in range(C))
        x = np.linalg.solve(Sw / n, means.T)                         # (a+1, C): Sigma^-1 m_c
        coef[a] = Va @ x
        icpt[a] = -0.5 * np.sum(means.T * x, axis=0) + np.log(np.bincount(yt, minlength=C) / n)
    return coef, icpt, sv ** 2, (mu, sd)


def e2e_reference(X, y, w, folds, C, A, scale=False):
    """(scores (N, A, C) with NaN for rows in no fold, allowed (N, A): the error allowed on a difference of two
    scores of that row, ratios (F, A): lambda_a / lambda_{a+1}).

    The allowed error.  The device's models are held to the gate against the truth on the device's own
    eigenpairs: ||d coef|| <= b_c ||coef||, |d intercept| <= b_i max |intercept|, b = 2 Y + c u of this design's
    Reference; a difference of two classes' errors is at most sqrt(2) times the norm of the error vector; the
    prediction kernel's dot product adds K + 2 roundings relative to |z| . |coef_c| and the standardised row
    differs from the device's by a few roundings per element (4 u).  The device's eigenpairs are those of its own
    eigensolver, whose backward error is 32 K u ||XTX|| (pcr.py's rank_tol): the subspace of the first a + 1
    components turns by at most theta_a = 32 K u lambda_0 / (lambda_a - lambda_{a+1}) (Davis-Kahan), and with
    coef_a = n V_a S_a^-1 V_a^T (H / n_c) a turn E of V_a changes coef by n [E S^-1 M~ + V S^-1 E^T H / n_c
    - V S^-1 (E^T T V + V^T T E) S^-1 M~], T the within-class scatter with ||T|| <= lambda_0: at most
    theta_a (1 + 3 chi_a) ||coef_a|| with chi_a = lambda_0 ||S_a^-1||; the intercepts move by as much relative to
    n m~ . S^-1 m~, which is bounded by twice their largest magnitude."""
    N, K = X.shape
    scores = np.full((N, A, C), np.nan)
    allowed = np.full((N, A), np.nan)
    ratios = np.zeros((len(folds), A))
    V, E, nc, XTY, CW = batch_inputs(X, y, w, folds, C, A, scale=scale)
    ref = Reference(V, E, nc, XTY, CW)
    XTX = lc.batch_inputs(X, y, w, folds, C, scale=scale)[0]
    for f, val in enumerate(folds):
        coef, icpt, lam, (mu, sd) = row_reference_fold(X, y, w, val, C, A, scale)
        ratios[f] = lam[:A] / lam[1:A + 1]
        Z = (X[val] - mu) / sd
        zn = np.linalg.norm(Z, axis=1)
        _, S, _ = scatter_ld(V[f], E[f], XTY[f], CW[f])
        S = S.astype(np.float64)
        lam_all = np.linalg.eigvalsh(XTX[f])[::-1]
        for a in range(A):
            scores[val, a] = Z @ coef[a] + icpt[a]
            bc, bi = ref.bounds(a)
            theta = 32.0 * K * U * lam_all[0] / (lam_all[a] - lam_all[a + 1])
            chi = lam_all[0] * np.linalg.norm(np.linalg.inv(S[:a + 1, :a + 1]), 2)
            turn = theta * (1.0 + 3.0 * chi)
            cn, imax = np.linalg.norm(coef[a]), np.abs(icpt[a]).max()
            dots = np.abs(Z) @ np.abs(coef[a])
            allowed[val, a] = np.sqrt(2.0) * (zn * (bc + turn + 4 * U) * cn + (bi + 2.0 * turn) * imax * np.sqrt(C)) \
                + 2.0 * (K + 2) * U * dots.max(axis=1)
    return scores, allowed, ratios


def decided_rows(scores, allowed):
    """(labels (N, A) with -1 for rows in no fold, decided (N, A) bool): tests/lda_cases.decided_rows."""
    return lc.decided_rows(scores, allowed)
