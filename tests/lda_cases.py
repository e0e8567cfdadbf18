"""Designs, the reference and the accuracy gate of the device-LDA tests (tests/test_gpu_lda.py on the GPU;
tests/test_lda_host.py checks on the CPU that every design meets its own conditions and that the NumPy
restatement below is scikit-learn's lsqr LDA).  NumPy and the oracle only: nothing here touches the product.

Reference.  The within-class scatter is summed from class-centred training rows (no cancellation: every term
is a square or a product of deviations from the class's own mean) and ``(S_w + lambda tr S_w / K I) x = m_c`` is
solved by ``oracle.ridge_oracle.ridge_solve_ref``; S_w is not rescaled first, so the matrix the oracle solves
carries no rounding but that of its own sums.

Yardstick.  ``restate`` is the kernel's route in plain NumPy float64: the rank-C downdate of the fold's XTX,
the scaling to trace K, ``numpy.linalg.solve``.  Y is its relative Frobenius error against the reference.

Gate.  ``err <= 2 Y + c u`` (float32: plus the one rounding of the store), the largest Y over the folds of a
batch, for ``coef`` and for the differences of ``intercept`` between present classes.  c counts the roundings
the device makes and the yardstick's error does not stand for:
  * the downdate: an entry of S_w is XTX_ij - sum_c m_c[i] h_c[j] with m_c = h_c / n_c rounded once and one
    fused multiply-add per class, then the subtraction and the scaling by K / tr S_w: 2 C + 2 roundings, each
    relative to a term of the size of XTX_ij while the result has the size of S_w -- times the cancellation
    factor kappa = ||XTX||_F / ||S_w||_F of the fixture;
  * the finish: 1 - g, lambda = g / (1 - g), K / tr S_w, n K / tr S_w, the division by 1 - g, the product
    with x: 8 roundings with the two of log(n_c / n);
  * the intercept's dot product m_c . coef_c of K terms, summed in some fixed order: at most K + 2 roundings
    relative to sum |m_c[k] coef_c[k]|, which the gate on the intercepts adds relative to the norm of the
    differences it measures.
A float32 store rounds every element by 2^-24 of itself: 2^-24 of the norm for coef; for the differences of the
intercepts 2^-24 (||intercept|| + sqrt(P - 1) |intercept[first]|) over the norm of the differences."""

import os

import numpy as np

from oracle import ridge_oracle as ro

U = ro.U
GAMMAS = np.array([0.0, 0.1, 0.5, 1.0])
N_FOLDS = 3

K_VALUES = (1, 2, 31, 32, 33, 64, 257)
C_VALUES = (2, 3, 17, 64)
# (K, C): every K, every C; both sides of the 32-wide tile, the 64-class limit at K below, at and above a tile
GRID = [(1, 2), (1, 3), (1, 64), (2, 2), (2, 17), (31, 2), (31, 3), (31, 64), (32, 2), (32, 17), (32, 64),
        (33, 3), (33, 17), (33, 64), (64, 2), (64, 3), (64, 64), (257, 2), (257, 17), (257, 64)]
GRID_F32 = [(1, 2), (2, 17), (31, 64), (33, 3), (64, 64), (257, 17)]

LADDER_KC = (33, 3)
LADDER_SEP = (1.0, 1e2, 1e4)


# ---- designs

def make_rows(seed, N, K, C, sep=1.0, integer_weights=False):
    """N rows of K variables in C classes: unit within-class standard deviation, class means ``sep`` within-class
    standard deviations apart (random directions of length sep), an offset so that centring matters, labels
    dealt in rounds of C + 1 with class 0 twice in a round: the classes are not balanced (between two balanced
    classes the intercepts do not differ, and their difference could not be held against anything).
    ``integer_weights``: weights 1..3, else None."""
    rng = np.random.default_rng(seed)
    y = (np.arange(N) % (C + 1)) % C
    d = rng.standard_normal((C, K))
    means = sep * d / np.linalg.norm(d, axis=1, keepdims=True)
    X = rng.standard_normal((N, K)) + means[y] + 0.5
    w = rng.integers(1, 4, N).astype(np.float64) if integer_weights else None
    return X, y, w


def folds_of(N, C, F=N_FOLDS):
    """F validation sets: the rows in their rounds of C + 1 (every class in each), round b in fold b % F.  With
    F rounds and more, every fold validates and trains on every class."""
    return [np.flatnonzero((np.arange(N) // (C + 1)) % F == f) for f in range(F)]


def grid_rows(K, C):
    """The rows of a shape-grid case: every training set (two thirds of the rows) holds 4 (K + C) rows and more,
    so S_w (rank: rows minus classes) is positive definite with room."""
    N = 6 * (K + C) + 45
    return make_rows(1000 * K + C, N, K, C)


def ladder_rows(sep):
    K, C = LADDER_KC
    return make_rows(int(sep), 6 * (K + C) + 45, K, C, sep=sep)


def indicator(y, C):
    Y = np.zeros((y.size, C))
    Y[np.arange(y.size), y] = 1.0
    return Y


def training_stats(X, w, val, scale=False, ddof=1):
    """(training rows, their weights, weighted mean, std or ones) as the fold stage forms them."""
    tr = np.setdiff1d(np.arange(X.shape[0]), val)
    wt = np.ones(tr.size) if w is None else w[tr]
    mu = (wt @ X[tr]) / wt.sum()
    sd = np.ones(X.shape[1])
    if scale:
        nz = np.count_nonzero(wt)
        sd = np.sqrt((wt @ (X[tr] - mu) ** 2) * nz / ((nz - ddof) * wt.sum()))
    return tr, wt, mu, sd


def fold_inputs(X, y, w, val, C, scale=False):
    """What the device is handed for one fold, formed in float64: XTX (symmetric), XTY, class weights."""
    tr, wt, mu, sd = training_stats(X, w, val, scale)
    Z = (X[tr] - mu) / sd
    XTX = Z.T @ (wt[:, None] * Z)
    Yt = indicator(y[tr], C)
    return 0.5 * (XTX + XTX.T), Z.T @ (wt[:, None] * Yt), wt @ Yt


def batch_inputs(X, y, w, folds, C, dtype=np.float64, scale=False):
    """(XTX (F,K,K), XTY (F,K,C) in ``dtype``, class weights (F,C) float64) for a list of validation index arrays."""
    parts = [fold_inputs(X, y, w, val, C, scale) for val in folds]
    return (np.stack([p[0] for p in parts]).astype(dtype), np.stack([p[1] for p in parts]).astype(dtype),
            np.stack([p[2] for p in parts]))


# ---- the reference

def reference_fold(X, y, w, val, C, gammas=GAMMAS, scale=False):
    """coef (L,K,C), intercept (L,C), the class weights (C,), S_w (K,K) of one fold from its training rows.
    An absent class has coef 0 and intercept -inf.  g = 0 on a singular S_w raises ``LinAlgError`` (the
    oracle's Cholesky)."""
    tr, wt, mu, sd = training_stats(X, w, val, scale)
    Z = (X[tr] - mu) / sd
    yt = y[tr]
    K = Z.shape[1]
    n = wt.sum()
    cw = np.array([wt[yt == c].sum() for c in range(C)])
    Sw = np.zeros((K, K))
    M = np.zeros((K, C))
    for c in range(C):
        if cw[c] > 0:
            Zc, wc = Z[yt == c], wt[yt == c]
            mc = (wc @ Zc) / cw[c]
            D = Zc - mc
            Sw += D.T @ (wc[:, None] * D)
            M[:, c] = mc - (wt @ Z) / n
    Sw = 0.5 * (Sw + Sw.T)
    t = np.trace(Sw) / K
    coef = np.zeros((len(gammas), K, C))
    icpt = np.full((len(gammas), C), -np.inf)
    present = cw > 0
    for l, g in enumerate(gammas):
        coef[l] = n / (1.0 - g) * ro.ridge_solve_ref(Sw, M, g / (1.0 - g) * t) if g < 1.0 else (n / t) * M
        coef[l][:, ~present] = 0.0
        icpt[l, present] = -0.5 * np.sum(M * coef[l], axis=0)[present] + np.log(cw[present] / n)
    return coef, icpt, cw, Sw


def reference_batch(X, y, w, folds, C, gammas=GAMMAS, scale=False):
    parts = [reference_fold(X, y, w, val, C, gammas, scale) for val in folds]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


# ---- the yardstick: the kernel's route in NumPy

def restate(XTX, XTY, cw, gammas=GAMMAS):
    """coef (L,K,C), intercept (L,C) of one fold by the downdate of XTX, the scaling to trace K and
    ``numpy.linalg.solve`` (float32 inputs widened first, which is exact)."""
    XTX = np.asarray(XTX, dtype=np.float64)
    XTY = np.asarray(XTY, dtype=np.float64)
    K, C = XTY.shape
    present = cw > 0
    M = np.zeros((K, C))
    M[:, present] = XTY[:, present] / cw[present]
    Sw = XTX - M @ XTY.T
    n = cw.sum()
    s = K / np.trace(Sw)
    Sp = s * Sw
    coef = np.zeros((len(gammas), K, C))
    icpt = np.full((len(gammas), C), -np.inf)
    for l, g in enumerate(gammas):
        if g < 1.0:
            coef[l] = (n * s) / (1.0 - g) * np.linalg.solve(Sp + g / (1.0 - g) * np.eye(K), M)
        else:
            coef[l] = (n * s) * M
        coef[l][:, ~present] = 0.0
        icpt[l, present] = -0.5 * np.sum(M * coef[l], axis=0)[present] + np.log(cw[present] / n)
    return coef, icpt


# ---- the gate

def icpt_differences(icpt, present):
    """The intercepts of the present classes minus that of the first of them (the first itself left out)."""
    d = np.asarray(icpt, dtype=np.float64)[..., present]
    return d[..., 1:] - d[..., :1]


def kappa(XTX, Sw):
    """The cancellation factor of the downdate, the largest over the folds."""
    XTX = np.asarray(XTX, dtype=np.float64)
    return max(np.linalg.norm(XTX[f]) / np.linalg.norm(Sw[f]) for f in range(XTX.shape[0]))


def gate_c(C, kap):
    return (2 * C + 2) * kap + 8


def yardsticks(XTX, XTY, CW, ref_coef, ref_icpt, gammas=GAMMAS):
    """(Y for coef (L,), Y for the intercept differences (L,)): the largest over the folds."""
    F, L = ref_coef.shape[:2]
    Yc, Yi = np.zeros(L), np.zeros(L)
    for f in range(F):
        coef, icpt = restate(XTX[f], XTY[f], CW[f], gammas)
        present = CW[f] > 0
        for l in range(L):
            Yc[l] = max(Yc[l], ro.rel_err(coef[l], ref_coef[f, l]))
            Yi[l] = max(Yi[l], ro.rel_err(icpt_differences(icpt[l], present),
                                          icpt_differences(ref_icpt[f, l], present)))
    return Yc, Yi


def coef_bound(Y, c, float32=False):
    return (2.0 ** -24 if float32 else 0.0) + 2.0 * Y + c * U


def icpt_bound(Y, c, ref_coef, ref_icpt, M, present, float32=False):
    """The bound on the relative error of the intercept differences of one model: the gate, the dot product's
    K + 2 roundings and (float32) the store, the last two relative to the norm of the differences."""
    d = np.linalg.norm(icpt_differences(ref_icpt, present))
    K = ref_coef.shape[0]
    dots = np.sum(np.abs(M * ref_coef), axis=0)[present]
    b = 2.0 * Y + c * U + (K + 2) * U * (np.linalg.norm(dots) + np.sqrt(dots.size - 1) * dots[0]) / d
    if float32:
        ic = np.abs(ref_icpt[present])
        b += 2.0 ** -24 * (np.linalg.norm(ic) + np.sqrt(ic.size - 1) * ic[0]) / d
    return b


def assert_gate(coef, icpt, XTX, XTY, CW, refs, what, gammas=GAMMAS, float32=False):
    """Every model of the batch against the gate; returns the largest err / Y over coef and intercepts.
    CVM_LDA_REPORT=path: one line per comparison."""
    ref_coef, ref_icpt, _, Sw = refs
    coef = np.asarray(coef, dtype=np.float64)
    icpt = np.asarray(icpt, dtype=np.float64)
    F, L, K, C = ref_coef.shape
    c = gate_c(C, kappa(XTX, Sw))
    Yc, Yi = yardsticks(XTX, XTY, CW, ref_coef, ref_icpt, gammas)
    report = os.environ.get("CVM_LDA_REPORT")
    lines, bad, worst = [], [], 0.0
    for f in range(F):
        present = CW[f] > 0
        M = np.zeros((K, C))
        M[:, present] = np.asarray(XTY[f], dtype=np.float64)[:, present] / CW[f][present]
        for l in range(L):
            ec = ro.rel_err(coef[f, l], ref_coef[f, l])
            ei = ro.rel_err(icpt_differences(icpt[f, l], present), icpt_differences(ref_icpt[f, l], present))
            bc = coef_bound(Yc[l], c, float32)
            bi = icpt_bound(Yi[l], c, ref_coef[f, l], ref_icpt[f, l], M, present, float32)
            worst = max(worst, ec / Yc[l] if Yc[l] > 0 else 0.0, ei / Yi[l] if Yi[l] > 0 else 0.0)
            lines.append(f"{what} f={f} g={gammas[l]:g}\tcoef {ec:.3e} Y {Yc[l]:.3e} bound {bc:.3e}\t"
                         f"intercept {ei:.3e} Y {Yi[l]:.3e} bound {bi:.3e}\n")
            if not (ec <= bc and ei <= bi):
                bad.append(lines[-1].strip())
    if report:
        with open(report, "a") as fh:
            fh.writelines(lines)
    assert not bad, f"{what}: error above 2 Y + {c:.3g} u" + (" + 2^-24" if float32 else "") + ": " + "; ".join(bad[:6])
    return worst


# ---- the special designs

def absent_case():
    """K = 33, C = 4, 3 folds: every row of class 2 lies in fold 1's validation set, so fold 1 trains without
    class 2 and the other folds with all four classes."""
    K, C, N = 33, 4, 240
    X, y, _ = make_rows(77, N, K, C)
    order = np.concatenate([np.flatnonzero(y == 2), np.flatnonzero(y != 2)])
    n2 = int(np.sum(y == 2))
    rest = order[n2:]
    folds = [np.sort(rest[0::2][:60]), np.sort(np.concatenate([order[:n2], rest[1::2][:20]])),
             np.sort(rest[1::2][20:80])]
    return X, y, folds, C


def singular_case():
    """K = 40, C = 3, 3 folds of which fold 1 trains on 30 rows (rank of S_w at most 27): its validation set is
    everything but those 30.  The other two folds train on 140 rows and more."""
    K, C, N = 40, 3, 210
    X, y, _ = make_rows(40, N, K, C)
    folds = [np.arange(0, 70), np.arange(30, N), np.arange(140, 210)]
    return X, y, folds, C


def zero_trace_inputs(K=8, C=3):
    """One fold's inputs where every row equals its class mean: XTX is exactly sum_c n_c m_c m_c^T in small
    integers, so the downdate gives exactly zero."""
    rng = np.random.default_rng(5)
    means = rng.integers(-3, 4, (C, K)).astype(np.float64)
    cw = np.array([4.0, 2.0, 2.0])[:C]
    means -= (cw @ means) / cw.sum()                    # centred: multiples of 1/8, every product exact
    XTY = (means * cw[:, None]).T
    XTX = (means.T * cw) @ means
    return XTX, XTY, cw


# ---- end to end

E2E = dict(N=600, K=12, C=4, F=5)
E2E_SKIP_CAP = 0.01


def e2e_rows(weighted):
    X, y, w = make_rows(600 + int(weighted), E2E["N"], E2E["K"], E2E["C"], sep=3.0, integer_weights=weighted)
    labels = (np.arange(E2E["N"]) // (E2E["C"] + 1)) % (E2E["F"] + 1)       # label F: rows in no fold
    folds = [np.flatnonzero(labels == f) for f in range(E2E["F"])]
    return X, y, w, folds, np.flatnonzero(labels == E2E["F"])


def reference_scores(X, y, w, folds, C, gammas=GAMMAS, scale=False):
    """(scores (N, L, C) with NaN for rows in no fold, allowed (N, L): the error the gate allows on a difference
    of two scores of that row) from the reference of every fold.  A score is z . coef_c + intercept_c; the gate
    bounds ||d coef||_F by b_c ||coef||_F and the norm of the intercept differences' error by b_i times their
    norm; a difference of two classes' errors is at most sqrt(2) times the norm of the error vector; the
    prediction kernel's own dot product adds K + 2 roundings relative to |z| . |coef_c|, and the standardised
    row differs from the device's by a few roundings per element (4 u)."""
    N, K = X.shape
    L = len(gammas)
    scores = np.full((N, L, C), np.nan)
    allowed = np.full((N, L), np.nan)
    refs = reference_batch(X, y, w, folds, C, gammas, scale)
    XTX, XTY, CW = batch_inputs(X, y, w, folds, C, scale=scale)
    c = gate_c(C, kappa(XTX, refs[3]))
    Yc, Yi = yardsticks(XTX, XTY, CW, refs[0], refs[1], gammas)
    for f, val in enumerate(folds):
        _, _, mu, sd = training_stats(X, w, val, scale)
        Z = (X[val] - mu) / sd
        present = CW[f] > 0
        M = np.zeros((K, C))
        M[:, present] = XTY[f][:, present] / CW[f][present]
        for l in range(L):
            coef, icpt = refs[0][f, l], refs[1][f, l]
            scores[val, l] = Z @ coef + icpt
            bc = coef_bound(Yc[l], c)
            bi = icpt_bound(Yi[l], c, coef, icpt, M, present)
            zn = np.linalg.norm(Z, axis=1)
            dots = np.abs(Z) @ np.abs(coef)
            allowed[val, l] = np.sqrt(2.0) * (zn * (bc + 4 * U) * np.linalg.norm(coef)
                                              + bi * np.linalg.norm(icpt_differences(icpt, present))) \
                + 2.0 * (K + 2) * U * dots.max(axis=1)
    return scores, allowed


def decided_rows(scores, allowed):
    """(labels (N, L) with -1 for rows in no fold, decided (N, L) bool: the gap between the two largest scores
    exceeds the allowed error)."""
    N, L, C = scores.shape
    none = np.isnan(scores[:, :, 0])
    s = np.where(np.isnan(scores), -np.inf, scores)
    top = np.sort(s, axis=2)
    with np.errstate(invalid="ignore"):
        margin = top[:, :, -1] - top[:, :, -2]
    labels = np.where(none, -1, np.argmax(s, axis=2))
    return labels, (margin > allowed) & ~none
