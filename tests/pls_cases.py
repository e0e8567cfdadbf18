"""Case builders, the reference side and the gates of the extended device-PLS tests
(tests/test_gpu_pls_extended.py on the GPU; tests/test_pls_extended_oracle.py checks on the CPU that every
builder meets its own conditions).  NumPy and the oracle only; ``plan`` asks the library's host-side planner
(no GPU needed: it then assumes 256 CUs).  Everything is seeded and small."""

import numpy as np

from oracle.ikpls_oracle import ikpls_fit, ikpls_follow

U = 2.0 ** -53
YARDSTICK_CAP = 1e-13            # every designed case keeps its yardstick below this for all its components

ONE = "one workgroup per fold"
REP = "replicated small state, one barrier per component"
FOUR = "row slices, four barriers per component"

# (a) the route table: (F, K, M, A, dtype, kernel, slices, XTX slice in LDS) -- the smallest shapes that reach
# each route, ragged last slices and the padding blocks of the one-barrier grid included
ROUTES = [
    (300, 24, 3, 6, np.float64, ONE, 1, True),
    (300, 33, 5, 6, np.float64, ONE, 1, True),        # odd K: the scalar loads
    (300, 136, 2, 6, np.float64, ONE, 1, False),      # XTX streamed
    (1, 25, 2, 3, np.float64, REP, 4, False),
    (9, 33, 2, 6, np.float64, REP, 5, False),         # rows 7: ragged last slice, 7 padding folds in the XCD grid
    (56, 40, 3, 4, np.float64, REP, 4, False),
    (57, 40, 3, 4, np.float64, ONE, 1, True),         # one fold too many for S = 4
    (2, 1028, 1, 4, np.float64, FOUR, 115, True),     # rows 9, ragged, M = 1
    (4, 1032, 2, 4, np.float64, FOUR, 61, False),
    (3, 512, 64, 5, np.float64, FOUR, 64, True),      # XTY too wide for the one-barrier route
    (64, 448, 4, 5, np.float64, FOUR, 4, False),
]
ROUTE_F32 = (60, 768, 4, 5, np.float32, FOUR, 4, False)
# the M classes of the eigen code (registers 1 x 1 and 2 x 2 blocks, LDS 3 x 3 and 4 x 4) on two routes
M_CLASSES = (1, 2, 16, 17, 32, 33, 48, 49, 64)
M_CLASS_ROUTES = [(300, 72, ONE), (5, 40, REP)]        # (F, K, kernel), A = 3 (K = 40: M = 64 still fits the one-barrier LDS plan)
DISTINCT = 6                                            # distinct matrices in a stack of many folds

LADDER_COND = (1e2, 1e6, 1e10)
LADDER_SHAPES = [(5, 32, 3, 10), (3, 520, 3, 10)]       # (F, K, M, A): K = 32 and one sliced shape
GAPS = (0.5, 1e-3, 1e-6, 1e-9, 1e-12, 0.0)
GAP_M = (2, 5, 16, 33, 64)
GAP_K, GAP_A = 72, 3


def plan(F, K, M, A, dtype=np.float64):
    from cvmatrix_amd.pls import pls_plan
    return pls_plan(F, K, M, A, dtype)


def assert_plan(F, K, M, A, dtype, kernel, slices=None, xtx_in_lds=None):
    p = plan(F, K, M, A, dtype)
    assert p["kernel"] == kernel, (F, K, M, A, p)
    if slices is not None:
        assert p["slices"] == slices, (F, K, M, A, p)
    if xtx_in_lds is not None:
        assert p["xtx_in_lds"] == xtx_in_lds, (F, K, M, A, p)
    return p


def rel(a, b):
    """Relative Frobenius error, computed in the wider of the two types."""
    a, b = np.asarray(a), np.asarray(b)
    d = (a.astype(np.longdouble) - b.astype(np.longdouble)).ravel()
    n = b.astype(np.longdouble).ravel()
    return float(np.sqrt(d @ d) / max(np.sqrt(n @ n), np.longdouble(1e-300)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def folds(seed, n, K, M, cond=1e2, dtype=np.float64):
    """n distinct folds (XTX (n,K,K) symmetric to the bit and positive definite, XTY (n,K,M)) from data
    X (2K + 3 rows) whose column scales are spread over sqrt(cond): cond(XTX) is cond times the few tens of
    a random tall matrix.  Y = X B + noise.  float32: rounded from the float64 matrices (still symmetric)."""
    rng = np.random.default_rng(seed)
    scales = cond ** (-np.arange(K) / (2.0 * max(K - 1, 1)))
    XTX = np.empty((n, K, K))
    XTY = np.empty((n, K, M))
    for f in range(n):
        X = rng.standard_normal((2 * K + 3, K)) * scales
        Y = X @ rng.standard_normal((K, M)) + 0.1 * rng.standard_normal((2 * K + 3, M))
        G = X.T @ X
        XTX[f] = 0.5 * (G + G.T)
        XTY[f] = X.T @ Y
    return XTX.astype(dtype), XTY.astype(dtype)


def pattern(F, n):
    """Which distinct matrix fold f of a stack holds: every one of the n occurs, neighbours differ, and the
    pattern has no period that divides 8 (the folds of the one-barrier grid are dealt over 8 XCDs)."""
    f = np.arange(F)
    return (3 * f + f // 7) % n


def route_case(F, K, M, A, dtype=np.float64, cond=1e2):
    """(XTX, XTY, idx): the stack of a route-table entry and the distinct matrix each fold holds."""
    n = min(F, DISTINCT)
    dX, dY = folds(100003 * K + 1009 * M + F, n, K, M, cond, dtype)
    idx = pattern(F, n)
    return dX[idx], dY[idx], idx


def gap_case(M, K=GAP_K, seed=0):
    """(c) one fold per gap g of GAPS: XTY = U diag(s) V^T with s_2 = s_1 sqrt(1 - g), the rest of s falling
    from 0.6 to 0.2, under a well-conditioned SPD XTX."""
    rng = np.random.default_rng(7000 + 10 * M + seed)
    XTX, _ = folds(7100 + M + seed, len(GAPS), K, 1)
    XTY = np.empty((len(GAPS), K, M))
    for i, g in enumerate(GAPS):
        Uo, _ = np.linalg.qr(rng.standard_normal((K, M)))
        Vo, _ = np.linalg.qr(rng.standard_normal((M, M)))
        s = np.concatenate([[1.0, np.sqrt(1.0 - g)], np.linspace(0.6, 0.2, max(M - 2, 0))])[:M]
        XTY[i] = (Uo * s) @ Vo.T
    return XTX, XTY


ZERO_FIRST = (40, 5, 3)                                  # K, M, A of zero_first_case


def zero_first_case(n=DISTINCT, seed=0):
    """The column pick of the squaring where it decides: XTY[0, 0] alone in its row and its column, so that
    XTY^T XTY is block diagonal to the bit, and half as large as the leading singular value of the other block:
    the dominant eigenvector has q_0 = 0 exactly, entry (0, 0) of the squared matrix dies out, and column 0 is
    the one column that holds nothing of q.  The column of the largest diagonal entry is unaffected."""
    K, M, _ = ZERO_FIRST
    rng = np.random.default_rng(9100 + seed)
    XTX, XTY = folds(9200 + seed, n, K, M)
    for f in range(n):
        XTY[f, 0, :] = 0.0
        XTY[f, :, 0] = 0.0
        XTY[f, 0, 0] = 0.5 * np.linalg.norm(XTY[f, 1:, 1:], 2) * (1.0 + 0.1 * rng.random())
    return XTX, XTY


def slice_rows(K, slices, rows):
    """A row of the first, of a middle and of the last slice of a plan (distinct where K allows)."""
    mid = min((slices // 2) * rows + min(1, rows - 1), K - 1) if slices > 1 else K // 2
    out = [0, mid, K - 1]
    assert len(set(out)) == 3, "the exhaustion and non-finite cases want K >= 3"
    return out


def exhaustion_case(F, K, M, A, slices, rows, dtype=np.float64):
    """(d) fold f has rank f mod (min(M, 3) + 1): XTX diagonal with powers of two, XTY with the values 3, 2, 1
    in its first `rank` columns, each alone in its row (a row of the first, a middle, the last slice).  Every
    step of the algorithm is then exact.  Returns the inputs and the closed-form outputs."""
    r3 = slice_rows(K, slices, rows)
    d = 2.0 ** ((np.arange(K) % 5) - 2)
    XTX = np.zeros((F, K, K))
    XTX[:, np.arange(K), np.arange(K)] = d
    XTY = np.zeros((F, K, M))
    B = np.zeros((F, A, K, M))
    W = np.zeros((F, K, A))
    Q = np.zeros((F, M, A))
    ranks = np.arange(F) % (min(M, 3) + 1)
    for f in range(F):
        for a in range(ranks[f]):
            v = 3.0 - a
            XTY[f, r3[a], a] = v
            W[f, r3[a], a] = 1.0                                 # w = r = p = e_row, tTt = d_row, q = v / d_row e_a
            Q[f, a, a] = v / d[r3[a]]
            B[f, a:, r3[a], a] = v / d[r3[a]]
        B[f, ranks[f]:] = 0.0
    t = lambda x: x.astype(dtype)                                # noqa: E731  (all values exact in float32)
    return t(XTX), t(XTY), {"B": t(B), "W": t(W), "P": t(W), "R": t(W), "Q": t(Q), "n_fit": ranks.astype(np.int32)}


def nonfinite_kinds(K, M, slices, rows):
    """(e) (name, poke): poke(XTX_f, XTY_f) makes one fold non-finite in place."""
    r3 = slice_rows(K, slices, rows)
    kinds = []
    for v, vn in ((np.nan, "nan"), (np.inf, "inf")):
        for r, c in ((r3[0], 0), (r3[1], M - 1), (r3[2], 0), (r3[2], M - 1)):
            kinds.append((f"xty_{vn}[{r},{c}]", lambda X, Y, r=r, c=c, v=v: Y.__setitem__((r, c), v)))

    def pair(X, Y):
        X[r3[1], r3[2]] = X[r3[2], r3[1]] = np.nan

    kinds.append((f"xtx_nan_pair[{r3[1]},{r3[2]}]", pair))
    for r in (r3[0], r3[2]):
        kinds.append((f"xtx_nan_diag[{r}]", lambda X, Y, r=r: X.__setitem__((r, r), np.nan)))

    kinds.append((f"xtx_inf_diag[{r3[1]}]", lambda X, Y, r=r3[1]: X.__setitem__((r, r), np.inf)))

    def whole(X, Y):
        X[...] = np.nan
        Y[...] = np.nan

    kinds.append(("all_nan", whole))
    return kinds


# ---- the reference side ------------------------------------------------------------------------------------

def orders(K):
    """Three orders of the K variables: as given, reversed, and a seeded shuffle."""
    return [np.arange(K), np.arange(K)[::-1].copy(), np.random.default_rng(K).permutation(K)]


def yardstick(XTX, XTY, W):
    """Y (A,): per component the error of the float64 restatement that follows W against the same code in
    longdouble, the largest over B, P, Q, R and over three orders of the variables.  Reference side only."""
    XTX, XTY, W = (np.asarray(x, dtype=np.float64) for x in (XTX, XTY, W))
    A = W.shape[1]
    Y = np.zeros(A)
    for o in orders(XTX.shape[0]):
        X_, Y_, W_ = np.ascontiguousarray(XTX[np.ix_(o, o)]), np.ascontiguousarray(XTY[o]), np.ascontiguousarray(W[o])
        lo = ikpls_follow(X_, Y_, W_, np.float64)
        hi = ikpls_follow(X_, Y_, W_, np.longdouble)
        for a in range(A):
            Y[a] = max(Y[a], rel(lo[0][a], hi[0][a]), *(rel(lo[i][:, a], hi[i][:, a]) for i in (1, 2, 3)))
    return Y


def case_yardstick(XTX, XTY, A):
    """The yardstick of a designed case: the largest over its distinct folds, W from the oracle's own
    squaring.  Also returns the oracle's largest Rayleigh deficit (M > 1)."""
    Y = np.zeros(A)
    worst_def = 0.0
    for f in range(XTX.shape[0]):
        X64, Y64 = XTX[f].astype(np.float64), XTY[f].astype(np.float64)
        *_, n = fit = ikpls_fit(X64, Y64, A, eig="squaring")
        assert n == A, (f, n, A)
        Y = np.maximum(Y, yardstick(X64, Y64, fit[1]))
        if XTY.shape[2] > 1:
            ref = ikpls_follow(X64, Y64, fit[1])
            worst_def = max(worst_def, max(deficits(ref[5], fit[1])))
    return Y, worst_def


def gate(Y):
    return 2.0 * Y + 4.0 * U


def deficits(Ys, W):
    """1 - |Y_a^T w_a|^2 / (|w_a|^2 lambda_max(Y_a^T Y_a)) per component: 0 for a dominant left singular
    vector of the deflated XTY before component a.  Everything in longdouble."""
    out = []
    for a in range(W.shape[1]):
        Ya = np.asarray(Ys[a], dtype=np.longdouble)
        w = np.asarray(W[:, a], dtype=np.longdouble)
        v = Ya.T @ w
        out.append(float(1.0 - (v @ v) / ((w @ w) * lambda_max(Ya.T @ Ya))))
    return out


def lambda_max(S):
    """The largest eigenvalue of the symmetric longdouble S: Rayleigh-Ritz in longdouble on LAPACK's two leading
    float64 eigenvectors (2 x 2, closed form).  What they miss of the leading eigenspace enters squared, and two
    leading eigenvalues a rounding apart -- where LAPACK's vectors are any basis of their plane -- are told apart."""
    if S.shape[0] == 1:
        return S[0, 0]
    V = np.linalg.eigh(S.astype(np.float64))[1][:, -2:].astype(np.longdouble)
    v1 = V[:, 1] / np.sqrt(V[:, 1] @ V[:, 1])
    v2 = V[:, 0] - (V[:, 0] @ v1) * v1
    v2 = v2 / np.sqrt(v2 @ v2)
    a, b, c = v1 @ (S @ v1), v1 @ (S @ v2), v2 @ (S @ v2)
    return (a + c) / 2 + np.sqrt(((a - c) / 2) ** 2 + b * b)


def deficit_slack(XTY, Ys):
    """64 u |XTY|_F / sigma_1(Y_a) per component: what the rounding of w = Y_a q alone may cost."""
    n0 = np.linalg.norm(np.asarray(XTY, dtype=np.float64))
    return [64 * U * n0 / np.linalg.norm(np.asarray(Ys[a], dtype=np.float64), 2) for a in range(Ys.shape[0])]
