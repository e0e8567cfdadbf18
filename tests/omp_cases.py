"""Helpers of the orthogonal matching pursuit tests (tests/test_omp_host.py on the CPU, tests/test_gpu_omp.py on
the device).  NumPy only; not collected.

The rule, for G = XTX[f], h = XTY[f][:, m], S the ordered list of selected indices, step a = 0 .. A - 1:

    1. alpha = h - G[:, S] gamma,  gamma the least-squares coefficients on S
    2. score_k = |alpha_k|  (normalize: |alpha_k| / sqrt(G_kk), columns whose G_kk is not > 0 left out),  k not in S
    3. j = the index of the largest score, the lowest index among equal scores; a largest score that is not > 0
       ends the path (scikit-learn stops where alpha_j^2 underflows)
    4. w = L^-1 G[S, j], d^2 = G_jj - w'w;  d^2 <= rank_tol G_jj ends the path
    5. L L' gamma = h_S

`reference` is that rule in plain NumPy -- Cholesky by np.linalg on G_SS afresh at every step, the scores in
np.longdouble -- and returns, per step, the SELECTION MARGIN: the best score minus the second best among the
candidates.  Two gates hold a device result against it:

  (1) support and n_fit equal the reference's exactly.  That is a fair demand only where every selection is
      decided beyond the rounding of alpha: `assert_decided` requires, at every step with n selected variables,
          margin >= 100 e,   e = max_k 8 (n + 2) u cond_2(G_SS) (|h_k| + (|G_kS| |gamma|)_k) scale_k + 4 u best score
      with u = 2^-53 -- alpha_k is a sum of n + 1 terms, and gamma carries the relative error of a Cholesky solve,
      about n u cond_2(G_SS); scale_k is 1, or 1 / sqrt(G_kk) with normalize, whose own rounding and the product's
      are the last term -- and cond_2(G_SS) <= 100.  The rescaled designs of normalize=True have column norms
      spread over 1 .. 30, so their cond_2(G_SS) reaches 900 times that of the plain design by the scaling alone;
      a Cholesky solve does not see a diagonal scaling (its errors are those of the equilibrated matrix), so there
      the demand cond <= 100 is made of D^-1/2 G_SS D^-1/2, D = diag(G_SS), while e keeps the plain (larger)
      cond_2(G_SS): the margin condition is the stricter for it.
  (2) for every step, with S its support, n = |S| and beta = B[f, a, S, m]:
          |h_S - G_SS beta| <= 2 (3 n + 1) u (|L^| |L^'| |beta|)      componentwise
      with L^ the reference's Cholesky factor of G_SS: the backward error of a Cholesky solve (Higham, Accuracy
      and Stability of Numerical Algorithms, Theorem 10.4), doubled.  float32 results add the rounding of the
      store carried through the residual, 2^-24 (|G_SS| |beta|).  The residual is evaluated in np.longdouble.
      Every entry of B[f, a, :, m] off S is exactly 0.

Neither bound was calibrated on what the kernel returns.

So that one reference serves the float64 and the float32 run of a case, the fixtures round G and h to float32 and
hand the float64 run the same numbers: the arithmetic under test is float64 either way (float32 inputs convert
exactly), only the store differs."""

import functools

import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -24
WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64

GRID_K = (1, 2, 63, 64, 65, 130, 257)
GRID_M = (1, 3, 17)
GRID_F = 3
MAX_SELECTED = 64
MARGIN_FACTOR = 100.0
COND_LIMIT = 100.0


def grid_A(K):
    """The steps of the grid at K: 1, min(K, 5), min(K, 64), without repeats."""
    return tuple(sorted({1, min(K, 5), min(K, MAX_SELECTED)}))


def default_rank_tol(A):
    return 32.0 * A * 2.0 ** -52


def rows_of(K, A):
    """Training rows of the grid's designs: 40 for K <= 2, else from 300 (one variable) to 1500 (64 variables), so
    that cond_2 of 64 selected columns stays below 4."""
    return 40 if K <= 2 else 300 + 1200 * (min(K, A) - 1) // 63


def design(n, K, M, A, seed=0, scaled=False):
    """Seeded X (n x K standard normal, centred; `scaled`: its columns multiplied by factors spread evenly in
    the logarithm over 1 .. 30, in a random order) and Y = X b + 0.5 noise, centred, with min(K, A) true
    coefficients per response (on the columns before they are rescaled) whose sizes fall from 3 to 1."""
    rng = np.random.default_rng([seed, n, K, M, A])
    X = rng.standard_normal((n, K))
    X -= X.mean(axis=0)
    t = min(K, A)
    b = np.zeros((K, M))
    for m in range(M):
        where = rng.permutation(K)[:t]
        b[where, m] = rng.choice([-1.0, 1.0], t) * np.linspace(3.0, 1.0, t)
    Y = X @ b + 0.5 * rng.standard_normal((n, M))
    if scaled:
        X = X * rng.permutation(np.geomspace(1.0, 30.0, K))
    return X, Y - Y.mean(axis=0)


@functools.lru_cache(maxsize=None)
def fold_matrices(n, K, M, A, F=GRID_F, seed=0, scaled=False):
    """(XTX (F,K,K), XTY (F,K,M)) float64 of F independent designs, every entry a float32 number; XTX symmetric
    to the bit.  Read-only."""
    XTX, XTY = np.empty((F, K, K)), np.empty((F, K, M))
    for f in range(F):
        X, Y = design(n, K, M, A, seed + 1000 * f, scaled)
        G = X.T @ X
        XTX[f], XTY[f] = 0.5 * (G + G.T), X.T @ Y
    XTX, XTY = XTX.astype(np.float32).astype(np.float64), XTY.astype(np.float32).astype(np.float64)
    XTX.setflags(write=False)
    XTY.setflags(write=False)
    return XTX, XTY


def score_scale(G, normalize):
    """(K,) WIDE: 1, or 1 / sqrt(G_kk) and 0 where G_kk is not > 0."""
    d = np.diag(G).astype(WIDE)
    if not normalize:
        return np.ones(d.size, WIDE)
    ok = d > 0
    return np.where(ok, 1 / np.sqrt(np.where(ok, d, 1)), 0)


def forward(L, b):
    """L x = b by substitution (np.linalg.solve would factor L afresh with row exchanges: not the solve gate 2
    is the bound of)."""
    x = np.empty(b.size)
    for i in range(b.size):
        x[i] = (b[i] - L[i, :i] @ x[:i]) / L[i, i]
    return x


def backward(L, b):
    """L' x = b by substitution."""
    x = np.empty(b.size)
    for i in range(b.size - 1, -1, -1):
        x[i] = (b[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_on(G, h, S):
    """(gamma, L): the least-squares coefficients on S by np.linalg's Cholesky factor of G_SS and two
    substitutions."""
    S = np.asarray(S, int)
    L = np.linalg.cholesky(G[np.ix_(S, S)])
    return backward(L, forward(L, h[S])), L


def reference(G, h, A, normalize=False, rank_tol=None):
    """One path.  Returns (support (A,) int, -1 padded; n_fit; coefficients (A, K), padded as the device pads;
    margins: n_fit floats, the best score minus the second best among the candidates of each selection, in units
    of the scores (inf where there was one candidate))."""
    G, h = np.asarray(G, np.float64), np.asarray(h, np.float64)
    K = h.size
    rank_tol = default_rank_tol(A) if rank_tol is None or rank_tol <= 0 else rank_tol
    scale = score_scale(G, normalize)
    S, margins = [], []
    coef = np.zeros((A, K))
    gamma, L = np.zeros(0), None
    for a in range(A):
        alpha = h.astype(WIDE) - G[:, S].astype(WIDE) @ gamma.astype(WIDE)
        score = np.abs(alpha) * scale
        cand = scale > 0
        cand[S] = False
        if not cand.any():
            break
        score = np.where(cand, score, -1)
        j = int(np.argmax(score))                       # (the first of equal scores: the lowest index)
        if not score[j] > 0:
            break
        if S:
            w = forward(L, G[S, j])
            d2 = G[j, j] - w @ w
        else:
            d2 = G[j, j]
        if d2 <= rank_tol * G[j, j]:
            break
        rest = np.delete(score, j)
        margins.append(float(score[j] - rest.max()) if cand.sum() > 1 else np.inf)
        S.append(j)
        gamma, L = solve_on(G, h, S)
        coef[a, S] = gamma
    n = len(S)
    for a in range(n, A):
        coef[a] = coef[n - 1] if n else 0.0
    support = np.full(A, -1, np.int64)
    support[:n] = S
    return support, n, coef, margins


def reference_batch(XTX, XTY, A, normalize=False, rank_tol=None):
    """(support (F,A,M), n_fit (F,M), B (F,A,K,M), margins {(f, m): list}) of `reference` on every path."""
    F, K, M = XTY.shape
    support, n_fit = np.empty((F, A, M), np.int64), np.empty((F, M), np.int64)
    B, margins = np.empty((F, A, K, M)), {}
    for f in range(F):
        for m in range(M):
            support[f, :, m], n_fit[f, m], B[f, :, :, m], margins[f, m] = reference(XTX[f], XTY[f][:, m], A, normalize, rank_tol)
    for a in (support, n_fit, B):
        a.setflags(write=False)
    return support, n_fit, B, margins


def decision_error(G, h, S, gamma, normalize):
    """(e, cond_2(G_SS), cond_2 of the equilibrated G_SS) for the selection that follows S (docstring, gate 1)."""
    n = len(S)
    scale = score_scale(G, normalize).astype(np.float64)
    if n == 0:
        mag, cond, cond_eq = np.abs(h), 1.0, 1.0
    else:
        GSS = G[np.ix_(S, S)]
        ev = np.linalg.eigvalsh(GSS)
        cond = float(ev[-1] / ev[0])
        r = 1.0 / np.sqrt(np.diag(GSS))
        ev = np.linalg.eigvalsh(GSS * np.outer(r, r))
        cond_eq = float(ev[-1] / ev[0])
        mag = np.abs(h) + np.abs(G[:, S]) @ np.abs(gamma)
    best = float((np.abs(h.astype(WIDE) - G[:, S].astype(WIDE) @ np.asarray(gamma, WIDE)) * scale).max())
    return float((8 * (n + 2) * U * cond * mag * scale).max()) + 4 * U * best, cond, cond_eq


def assert_decided(XTX, XTY, A, normalize, ref, scaled, what=""):
    """The condition gate 1 rests on, for every selection of every path of a case.  Returns (the smallest margin / e,
    the smallest margin / max|h|, the largest cond_2(G_SS), the largest equilibrated one)."""
    support, n_fit, B, margins = ref
    F, K, M = XTY.shape
    worst, rel, cmax, ceqmax = np.inf, np.inf, 1.0, 1.0
    for f in range(F):
        for m in range(M):
            G, h = XTX[f], XTY[f][:, m]
            for a in range(int(n_fit[f, m])):
                S = [int(v) for v in support[f, :a, m]]
                gamma = B[f, a - 1, S, m] if a else np.zeros(0)
                e, cond, cond_eq = decision_error(G, h, S, gamma, normalize)
                assert margins[f, m][a] >= MARGIN_FACTOR * e, (what, f, m, a, margins[f, m][a], e)
                assert (cond_eq if scaled else cond) <= COND_LIMIT, (what, f, m, a, cond, cond_eq)
                worst, cmax, ceqmax = min(worst, margins[f, m][a] / e), max(cmax, cond), max(ceqmax, cond_eq)
                rel = min(rel, margins[f, m][a] / (np.abs(h) * score_scale(G, normalize).astype(np.float64)).max())
            # the last selection of the path is followed by a step the gate covers too
            S = [int(v) for v in support[f, :int(n_fit[f, m]), m]]
            if S:
                ev = np.linalg.eigvalsh(G[np.ix_(S, S)])
                r = 1.0 / np.sqrt(np.diag(G)[S])
                eq = np.linalg.eigvalsh(G[np.ix_(S, S)] * np.outer(r, r))
                assert (eq[-1] / eq[0] if scaled else ev[-1] / ev[0]) <= COND_LIMIT, (what, f, m)
    return worst, rel, cmax, ceqmax


def second_gate(G, h, S, beta, float32=False):
    """(residual, bound), both (n,) float64: |h_S - G_SS beta| evaluated in WIDE and the right-hand side of gate 2."""
    S = np.asarray(S, int)
    n = S.size
    GSS = G[np.ix_(S, S)]
    L = np.abs(np.linalg.cholesky(GSS))
    ab = np.abs(np.asarray(beta, np.float64))
    res = np.abs(h[S].astype(WIDE) - GSS.astype(WIDE) @ np.asarray(beta, WIDE)).astype(np.float64)
    bound = 2 * (3 * n + 1) * U * (L @ (L.T @ ab))
    if float32:
        bound = bound + U32 * (np.abs(GSS) @ ab)
    return res, bound


def assert_second_gate(XTX, XTY, support, n_fit, B, float32=False, what=""):
    """Gate 2 and the exact zeros off the support, for every step of every path with n_fit >= 0 (the padding
    steps included: they repeat the last model).  Returns the largest attained fraction of the bound."""
    F, A, K, M = B.shape
    worst = 0.0
    for f in range(F):
        for m in range(M):
            n = int(n_fit[f, m])
            if n < 0:
                continue
            for a in range(A):
                S = support[f, :min(a + 1, n), m]
                b = B[f, a, :, m].astype(np.float64)
                off = np.ones(K, bool)
                off[S] = False
                assert np.all(b[off] == 0.0), f"{what}: fold {f} response {m} step {a}: a nonzero off the support"
                if S.size == 0:
                    continue
                assert np.all(np.isfinite(b)), (what, f, m, a)
                res, bound = second_gate(XTX[f], XTY[f][:, m], S, b[S], float32)
                i = int(np.argmax(res - bound))
                assert res[i] <= bound[i], f"{what} gate 2: fold {f} response {m} step {a} entry {i}: {res[i]:.3e} > {bound[i]:.3e}"
                worst = max(worst, float((res / np.maximum(bound, np.finfo(float).tiny)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def grid_case(K, M, A, normalize):
    """One case of the shape grid: (XTX, XTY, the reference batch).  normalize=True runs on the rescaled design."""
    XTX, XTY = fold_matrices(rows_of(K, A), K, M, A, seed=K + M, scaled=bool(normalize))
    return XTX, XTY, reference_batch(XTX, XTY, A, bool(normalize))


def tie_case():
    """G (8 x 8) and h built directly so that columns 2 and 5 are identical to the bit: row, column and the entry
    of h of index 2 duplicated into index 5.  The strongest true coefficient is on that column."""
    rng = np.random.default_rng(25)
    X = rng.standard_normal((60, 8))
    X -= X.mean(axis=0)
    X[:, 5] = X[:, 2]
    y = X @ np.array([0.5, -1.0, 2.0, 0.3, 0.0, 2.0, 0.7, -0.4]) + 0.1 * rng.standard_normal(60)
    G = X.T @ X
    G, h = 0.5 * (G + G.T), X.T @ (y - y.mean())
    G[5, :], G[:, 5], h[5] = G[2, :], G[:, 2], h[2]
    G[5, 5] = G[2, 2]
    assert np.array_equal(G[5], G[2]) and np.array_equal(G[:, 5], G[:, 2]) and np.array_equal(G, G.T)
    return G[None], h[None, :, None]


def low_rank_case(r=4, M=2, F=2):
    """2 r columns, the second half copies of the first to the bit: rank r."""
    XTX, XTY = np.empty((F, 2 * r, 2 * r)), np.empty((F, 2 * r, M))
    for f in range(F):
        X, Y = design(80, r, M, r, seed=77 + f)
        G = X.T @ X
        G, H = 0.5 * (G + G.T), X.T @ Y
        XTX[f], XTY[f] = np.block([[G, G], [G, G]]), np.concatenate([H, H])
    return XTX, XTY


def sklearn_cv_problem():
    """The end-to-end problem of the issue: N = 300, K = 24, M = 2, five folds, A = 6."""
    rng = np.random.default_rng(9)
    N, K, M, P = 300, 24, 2, 5
    X = rng.standard_normal((N, K)) + 0.5
    beta = np.zeros((K, M))
    beta[[1, 4, 7, 15, 20], 0] = [2.0, -1.5, 1.0, 0.8, -0.6]
    beta[[0, 4, 9, 11, 22, 23], 1] = [1.0, 1.2, -2.0, 0.5, 0.7, -0.9]
    Y = X @ beta + 0.3 * rng.standard_normal((N, M)) + 1.0
    return X, Y, np.arange(N) % P, 6
