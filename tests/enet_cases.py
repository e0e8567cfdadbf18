"""Helpers of the elastic net tests (tests/test_enet_host.py on the CPU, tests/test_gpu_enet.py on the device).
NumPy only.

The problem, for G = XTX[f], h = XTY[f][:, m], one penalty lam and one mixing value rho:

    minimise  1/2 b'Gb - h'b + lam (rho |b|_1 + 1/2 (1 - rho) |b|_2^2)

`reference_path` solves it by the cyclic coordinate rule of the device in plain NumPy; `kkt_violation` is the
optimality certificate; `assert_gates` holds a returned B against the two derived gates:

  (1) for every coordinate j,  v_j <= tol max|h| + 2 (K + 2) u (|h_j| + (|G||b|)_j + lam |b_j|),  u = 2^-53:
      the kernel's own stopping rule, plus the rounding of one freshly formed residual (a sum of K + 1 terms and
      the ridge term: (K + 2) u relative to the sum of the magnitudes), doubled.  float32 results add the rounding
      of the store carried through the residual, 2^-24 ((|G| + lam (1 - rho) I) |b|)_j;
  (2) with mu = lambda_min(G) + lam (1 - rho) > 0 and b* the reference:  |b - b*|_2 <= (|v(b)|_2 + |v(b*)|_2) / mu
      -- the objective is mu-strongly convex and v is its subgradient of least norm (float32: + 2^-24 |b|_2).

Neither bound was calibrated on what the kernel returns.

So that one reference serves the float64 and the float32 run of a case, the fixtures round G and h to float32
and hand the float64 run the same numbers: the arithmetic under test is float64 either way (float32 inputs
convert exactly), only the store differs."""

import functools

import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -24
WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64

GRID_K = (1, 3, 63, 64, 65, 130, 257)
GRID_M = (1, 3, 17)
GRID_RHO = (1.0, 0.5, 0.05)
GRID_FRACTIONS = np.array([0.5, 0.2, 0.1, 0.03, 0.01])      # of lambda_max: F = 3, L = 5
GRID_COND = 10.0
GPU_TOL = 1e-10                                               # the tol the device runs at in the gated tests
MAX_SWEEPS = 1000                                             # the default of enet_fit_batched
# the designs of the issue: (n, K, cond of X)
DESIGNS = ((200, 31, 1e2), (300, 64, 1e4), (400, 130, 1e2), (100, 96, 1e6))
DESIGN_RHO = (1.0, 0.5)
DESIGN_FRACTIONS = (0.5, 0.1, 0.01, 0.001)


def soft(z, t):
    return np.sign(z) * np.maximum(np.abs(z) - t, 0.0)


def design(n, K, cond, M=1, seed=0, nonzeros=5):
    """Seeded X = sqrt(n) U diag(s) V' (n x K, singular values log-spaced over `cond`, columns centred: U is an
    orthonormal basis of centred columns) and Y = X b + 0.1 noise, centred, with `nonzeros` true coefficients
    per response (every coefficient where nonzeros >= K)."""
    rng = np.random.default_rng([seed, n, K])
    Z = rng.standard_normal((n, K))
    Uo, _ = np.linalg.qr(Z - Z.mean(axis=0))
    V, _ = np.linalg.qr(rng.standard_normal((K, K)))
    s = np.logspace(0.0, -np.log10(cond), K) if K > 1 else np.ones(1)
    X = np.sqrt(n) * (Uo * s) @ V.T
    b = np.zeros((K, M))
    for m in range(M):
        where = rng.permutation(K)[:min(nonzeros, K)]
        b[where, m] = rng.choice([-1.0, 1.0], where.size) * rng.uniform(1.0, 3.0, where.size)
    Y = X @ b + 0.1 * rng.standard_normal((n, M))
    return X, Y - Y.mean(axis=0)


@functools.lru_cache(maxsize=None)
def fold_matrices(n, K, cond, M=1, F=1, seed=0, nonzeros=5, f32_exact=True):
    """(XTX (F,K,K), XTY (F,K,M)) float64 of F independent designs; XTX symmetric to the bit.  Read-only."""
    XTX, XTY = np.empty((F, K, K)), np.empty((F, K, M))
    for f in range(F):
        X, Y = design(n, K, cond, M, seed + 1000 * f, nonzeros)
        G = X.T @ X
        XTX[f], XTY[f] = 0.5 * (G + G.T), X.T @ Y
    if f32_exact:
        XTX, XTY = XTX.astype(np.float32).astype(np.float64), XTY.astype(np.float32).astype(np.float64)
    XTX.setflags(write=False)
    XTY.setflags(write=False)
    return XTX, XTY


def lambda_max(XTY, rho):
    """(F, M) as cvmatrix_amd.enet.lambda_max has it."""
    return np.abs(XTY).max(axis=-2) / rho


def kkt_violation(G, h, beta, lam, rho):
    """v (K,), float64, evaluated in np.longdouble where that is wider than double."""
    G, h, b = np.asarray(G, WIDE), np.asarray(h, WIDE), np.asarray(beta, WIDE)
    lam, rho = WIDE(lam), WIDE(rho)
    r = h - G @ b - lam * (1 - rho) * b
    v = np.where(b != 0, np.abs(r - lam * rho * np.sign(b)), np.maximum(0, np.abs(r) - lam * rho))
    return v.astype(np.float64)


def reference_path(G, H, lams, rho, tol=1e-12, max_sweeps=50000, snapshot_tol=None):
    """The cyclic coordinate rule in natural column order for every (penalty, response) of one fold, each from
    zero: (B (L,K,M), sweeps (L,M), converged (L,M)).  g = h - G b is updated by the row of G of every coefficient
    that moves and formed afresh after every sweep, when the certificate max_j v_j <= tol max|h| is looked at.
    `snapshot_tol` (looser than tol): also return (B, sweeps) as they were when each problem first passed the
    certificate at that tolerance -- what the same call with tol=snapshot_tol returns, without running it."""
    G, H, lams = np.asarray(G, np.float64), np.asarray(H, np.float64), np.asarray(lams, np.float64)
    K, M = H.shape
    L = lams.size
    lam = np.repeat(lams, M)                       # problem p = l * M + m
    hm = np.tile(H.T, (L, 1))                      # (P, K)
    lr, l2 = lam * rho, lam * (1.0 - rho)
    thr = tol * np.abs(hm).max(axis=1)
    b, g = np.zeros_like(hm), hm.copy()
    live = np.ones(lam.size, bool)
    sweeps = np.zeros(lam.size, np.int64)
    diag = np.diag(G)
    snap_b, snap_sweeps, snap_live = np.zeros_like(hm), np.zeros(lam.size, np.int64), np.ones(lam.size, bool)
    for _ in range(max_sweeps):
        for j in range(K):
            den = diag[j] + l2
            z = g[:, j] + diag[j] * b[:, j]
            bn = np.where(den > 0, soft(z, lr) / np.where(den > 0, den, 1.0), 0.0)
            delta = np.where(live, bn - b[:, j], 0.0)
            nz = delta != 0
            if nz.any():
                g[nz] -= np.outer(delta[nz], G[j])
                b[nz, j] = bn[nz]
        sweeps[live] += 1
        g[live] = hm[live] - b[live] @ G
        r = g - l2[:, None] * b
        v = np.where(b != 0, np.abs(r - lr[:, None] * np.sign(b)), np.maximum(0.0, np.abs(r) - lr[:, None]))
        if snapshot_tol is not None:
            now = snap_live & (v.max(axis=1) <= snapshot_tol / tol * thr)
            snap_b[now], snap_sweeps[now] = b[now], sweeps[now]
            snap_live &= ~now
        live &= ~(v.max(axis=1) <= thr)
        if not live.any():
            break
    shape = lambda a: a.reshape(L, M, K).transpose(0, 2, 1).copy()          # noqa: E731
    if snapshot_tol is not None:
        assert not snap_live.any() or live.any()
        return shape(b), sweeps.reshape(L, M), ~live.reshape(L, M), shape(snap_b), snap_sweeps.reshape(L, M)
    return shape(b), sweeps.reshape(L, M), ~live.reshape(L, M)


def first_gate_bound(G, h, beta, lam, rho, tol, float32=False):
    """(K,): the right-hand side of gate (1)."""
    K = h.size
    ab = np.abs(beta)
    bound = tol * np.abs(h).max() + 2 * (K + 2) * U * (np.abs(h) + np.abs(G) @ ab + lam * ab)
    if float32:
        bound = bound + U32 * (np.abs(G) @ ab + lam * (1 - rho) * ab)
    return bound


def strong_convexity(G, lam, rho):
    return float(np.linalg.eigvalsh(G)[0]) + lam * (1 - rho)


def distance_bound(G, h, beta, ref, lam, rho, float32=False, mu=None):
    """The right-hand side of gate (2)."""
    mu = strong_convexity(G, lam, rho) if mu is None else mu
    assert mu > 0, mu
    bound = (np.linalg.norm(kkt_violation(G, h, beta, lam, rho)) + np.linalg.norm(kkt_violation(G, h, ref, lam, rho))) / mu
    return bound + (U32 * np.linalg.norm(beta) if float32 else 0.0)


def assert_gates(XTX, XTY, lams, rho, tol, B, info, ref, float32=False, what="", only=None):
    """Both gates for every (f, l, m) with info == 0 (`only`: a boolean (F,L,M) mask of the problems to look at).
    Prints the largest ratio to each bound; returns the number of problems gated."""
    F, L, K, M = B.shape
    worst1 = worst2 = 0.0
    n = 0
    for f in range(F):
        lmin = float(np.linalg.eigvalsh(XTX[f])[0])
        for l in range(L):
            for m in range(M):
                if info[f, l, m] != 0 or (only is not None and not only[f, l, m]):
                    continue
                G, h, b = XTX[f], XTY[f][:, m], B[f, l, :, m].astype(np.float64)
                assert np.all(np.isfinite(b)), (what, f, l, m)
                v = kkt_violation(G, h, b, lams[l], rho)
                bound = first_gate_bound(G, h, b, lams[l], rho, tol, float32)
                j = int(np.argmax(v - bound))
                assert v[j] <= bound[j], f"{what} gate 1: fold {f} lambda {l} response {m} coordinate {j}: {v[j]:.3e} > {bound[j]:.3e}"
                worst1 = max(worst1, float((v / np.maximum(bound, np.finfo(float).tiny)).max()))
                d = np.linalg.norm(b - ref[f, l, :, m])
                db = distance_bound(G, h, b, ref[f, l, :, m], lams[l], rho, float32, mu=lmin + lams[l] * (1 - rho))
                assert d <= db, f"{what} gate 2: fold {f} lambda {l} response {m}: {d:.3e} > {db:.3e}"
                worst2 = max(worst2, d / db if db > 0 else 0.0)
                n += 1
    print(f"{what}: {n} problems; largest v / bound {worst1:.3f}, largest distance / bound {worst2:.3f}")
    return n


def support_is_decided(G, h, ref, lam, rho, tol):
    """Whether every solution that passes the certificate at `tol` has the reference's support: with the a-priori
    distance bound D = (tol max|h| sqrt(K) + |v(b*)|_2) / mu, a zero of b* stays zero when its margin
    lam rho - |r*_j| exceeds |G_j + lam (1 - rho) e_j|_2 D, a nonzero stays nonzero when |b*_j| > D."""
    K = h.size
    mu = strong_convexity(G, lam, rho)
    if not mu > 0:
        return False
    D = (tol * np.abs(h).max() * np.sqrt(K) + np.linalg.norm(kkt_violation(G, h, ref, lam, rho))) / mu
    r = h - G @ ref - lam * (1 - rho) * ref
    A = G + lam * (1 - rho) * np.eye(K)
    zero = ref == 0
    ok_zero = np.all((lam * rho - np.abs(r))[zero] > np.linalg.norm(A, axis=1)[zero] * D)
    return bool(ok_zero and np.all(np.abs(ref[~zero]) > D))


@functools.lru_cache(maxsize=None)
def grid_case(K, M, rho):
    """One case of the shape grid: (XTX, XTY, lambdas, reference B (F,L,K,M)).  F = 3, L = 5, the penalties
    GRID_FRACTIONS of the largest lambda_max, so every path starts inside the path of some problem."""
    n = 2 * K + 40
    XTX, XTY = fold_matrices(n, K, GRID_COND, M, 3, seed=K + M)
    lams = GRID_FRACTIONS * lambda_max(XTY, rho).max()
    ref = np.stack([reference_path(XTX[f], XTY[f], lams, rho)[0] for f in range(3)])
    ref.setflags(write=False)
    return XTX, XTY, lams, ref


def numpy_pipeline(X, Y, folds, lams, rho):
    """Centred, unweighted cross-validation in NumPy with the reference solver: out-of-fold predictions
    (L, N, M) and the validation SSE (F, L, M)."""
    N, M = Y.shape
    pred = np.zeros((len(lams), N, M))
    sse = np.zeros((len(folds), len(lams), M))
    for f, val in enumerate(folds):
        tr = np.setdiff1d(np.arange(N), val)
        mx, my = X[tr].mean(axis=0), Y[tr].mean(axis=0)
        Xc, Yc = X[tr] - mx, Y[tr] - my
        B = reference_path(Xc.T @ Xc, Xc.T @ Yc, lams, rho)[0]
        pred[:, val] = np.einsum("nk,lkm->lnm", X[val] - mx, B) + my
        sse[f] = ((pred[:, val] - Y[val]) ** 2).sum(axis=1)
    return pred, sse


# One case on each side of the kernel's route boundaries (cvmatrix_amd/csrc/enet.hpp): the active set holds 64
# coordinates (a dense solution at K = 64 fills it, at K = 65 overflows it into the fallback), and the LDS layout
# changes above K = 2048 (80 true nonzeros: both sides in the fallback, whose arrays are what the layout sizes).
# name: (n, K, true nonzeros, fractions of lambda_max, every coefficient nonzero at the smallest penalty)
ROUTE_CASES = {
    "dense64": (200, 64, 64, (0.1, 0.001), True),
    "dense65": (200, 65, 65, (0.1, 0.001), True),
    "wide2048": (256, 2048, 80, (0.3, 0.1), False),
    "wide2049": (256, 2049, 80, (0.3, 0.1), False),
}
ROUTE_RHO = 0.5


@functools.lru_cache(maxsize=None)
def route_case(name):
    """(XTX (1,K,K), XTY (1,K,1), lambdas, rho, reference B (1,L,K,1), dense).  The wide cases have fewer rows than
    columns (plain seeded normal columns, centred): rho = 0.5 keeps mu = lambda_min(G) + lambda / 2 > 0."""
    n, K, nonzeros, fractions, dense = ROUTE_CASES[name]
    if K <= 256:
        XTX, XTY = fold_matrices(n, K, GRID_COND, 1, 1, seed=K, nonzeros=nonzeros)
    else:
        rng = np.random.default_rng(K)
        X = rng.standard_normal((n, K))
        X -= X.mean(axis=0)
        b = np.zeros(K)
        where = rng.permutation(K)[:nonzeros]
        b[where] = rng.choice([-1.0, 1.0], nonzeros) * rng.uniform(1.0, 3.0, nonzeros)
        y = X @ b + 0.1 * rng.standard_normal(n)
        G = (X.T @ X).astype(np.float32).astype(np.float64)
        XTX, XTY = (0.5 * (G + G.T))[None], (X.T @ (y - y.mean())).astype(np.float32).astype(np.float64)[None, :, None]
    lams = np.array(fractions) * lambda_max(XTY, ROUTE_RHO).max()
    ref = reference_path(XTX[0], XTY[0], lams, ROUTE_RHO)[0][None]
    for a in (XTX, XTY, ref):
        a.setflags(write=False)
    return XTX, XTY, lams, ROUTE_RHO, ref, dense
