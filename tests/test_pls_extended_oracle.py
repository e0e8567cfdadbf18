"""CPU: the reference side of the extended device-PLS tests (tests/test_gpu_pls_extended.py) held to its
own conditions -- ``ikpls_follow`` pinned against 40-digit arithmetic and against ``ikpls_fit``,
``dominant_q_squaring`` on close and equal leading eigenvalues, the yardstick of every designed case below
its cap, the exhaustion fixture's closed form, and what the oracle makes of a non-finite fold.

Measured here (printed by the tests):
  mpmath pin: longdouble ikpls_follow within 7.2e-19 of 40 digits (B, P, Q, R, both shapes)
  dominant_q_squaring over the gap ladder: largest Rayleigh deficit 0.46 u
  largest yardstick of a designed case: 3.6e-15 (ladder, K = 32, cond 1e10); K >= 448: at most 3.3e-15"""

import numpy as np
import pytest

import pls_cases as pc
from oracle.ikpls_oracle import dominant_q_squaring, ikpls_fit, ikpls_follow

needs_longdouble = pytest.mark.skipif(not np.finfo(np.longdouble).eps < 2e-19, reason="np.longdouble is not the 80-bit format")


@pytest.mark.parametrize("K,M,A", [(4, 1, 3), (6, 3, 4)])
def test_follow_is_pinned_against_forty_digits(K, M, A):
    """The longdouble ikpls_follow against the same algorithm written out in mpmath at 40 digits, from the
    same weights.  Both run on well-conditioned tiny folds, where u (2^-64) grows by a small factor: 1e-17."""
    mp = pytest.importorskip("mpmath")
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is not the 80-bit format")
    XTX, XTY = pc.folds(40 + K, 1, K, M)
    XTX, XTY = XTX[0], XTY[0]
    W = ikpls_fit(XTX, XTY, A, eig="squaring")[1]
    got = ikpls_follow(XTX, XTY, W)
    mp.mp.dps = 40

    def to_mp(x):                                                # a longdouble as the exact sum of two doubles
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))

    X = mp.matrix(XTX.tolist())
    Y = mp.matrix(XTY.tolist())
    Wm = mp.matrix(W.tolist())
    Bm = mp.zeros(K, M)
    Rm, Pm = [], []
    worst = 0.0
    for a in range(A):
        w = Wm[:, a]
        r = w.copy()
        for j in range(a):
            r -= Rm[j] * (Pm[j].T * w)[0]
        u = X * r
        t = (r.T * u)[0]
        p = u / t
        q = (Y.T * r) / t
        Y = Y - (p * q.T) * t
        Bm = Bm + r * q.T
        Rm.append(r)
        Pm.append(p)
        for name, mine, ref in (("B", got[0][a], Bm), ("P", got[1][:, a], p), ("Q", got[2][:, a], q), ("R", got[3][:, a], r)):
            mine = np.asarray(mine).reshape(ref.rows, ref.cols)
            num = mp.sqrt(sum((to_mp(mine[i, j]) - ref[i, j]) ** 2 for i in range(ref.rows) for j in range(ref.cols)))
            den = mp.sqrt(sum(ref[i, j] ** 2 for i in range(ref.rows) for j in range(ref.cols)))
            e = float(num / den)
            worst = max(worst, e)
            assert e <= 1e-17, (name, a, e)
        assert abs(to_mp(got[4][a]) - t) / t <= 1e-17
    print(f"mpmath pin K={K} M={M}: worst {worst:.2e}")


@needs_longdouble
@pytest.mark.parametrize("eig", ["eigh", "squaring"])
@pytest.mark.parametrize("K,M,A", [(32, 3, 10), (33, 1, 6), (40, 17, 5)])
def test_follow_reproduces_the_fit(K, M, A, eig):
    XTX, XTY = pc.folds(K + M, 1, K, M, 1e6)
    B, W, P, Q, R, n = ikpls_fit(XTX[0], XTY[0], A, eig=eig)
    assert n == A
    lo = ikpls_follow(XTX[0], XTY[0], W, np.float64)
    for got, ref in zip(lo[:4], (B, P, Q, R)):
        assert pc.same_bits(got, ref)
    hi = ikpls_follow(XTX[0], XTY[0], W)
    Y = pc.yardstick(XTX[0], XTY[0], W)
    assert np.all(Y <= pc.YARDSTICK_CAP)
    for a in range(A):
        assert pc.rel(B[a], hi[0][a]) <= Y[a]
        assert np.array_equal(hi[5][0].astype(np.float64), XTY[0])


@needs_longdouble
def test_squaring_finds_a_dominant_vector_whatever_the_gap():
    """Close and equal leading eigenvalues: any vector of the leading eigenspace is right, so the vector is
    judged by its Rayleigh quotient.  The deficit of a unit q with an angle t to the eigenspace is below
    t^2; the polish and the normalisations round q by a few u, which moves the quotient by the same few u."""
    worst = 0.0
    for M in pc.GAP_M:
        _, XTY = pc.gap_case(M)
        for i, g in enumerate(pc.GAPS):
            S = XTY[i].T @ XTY[i]
            q = dominant_q_squaring(S).astype(np.longdouble)
            Sl = XTY[i].astype(np.longdouble).T @ XTY[i].astype(np.longdouble)
            assert abs(float(q @ q) - 1.0) <= 4 * pc.U
            d = float(1.0 - (q @ (Sl @ q)) / ((q @ q) * pc.lambda_max(Sl)))
            worst = max(worst, d)
            assert -2 * pc.U <= d <= 8 * pc.U, (M, g, d / pc.U)
    print(f"dominant_q_squaring: largest Rayleigh deficit {worst / pc.U:.2f} u")
    assert np.array_equal(dominant_q_squaring(np.zeros((3, 3))), np.zeros(3))
    # the lowest index among equal diagonal entries
    assert np.array_equal(dominant_q_squaring(np.eye(4)), np.array([1.0, 0, 0, 0]))


def designed_cases():
    for F, K, M, A, dtype, *_ in pc.ROUTES + [pc.ROUTE_F32]:
        yield f"route {F}x{K}x{M}x{A}", (lambda F=F, K=K, M=M, A=A, dtype=dtype: pc.route_case(F, K, M, A, dtype)[:2]), A
    for F, K, _ in pc.M_CLASS_ROUTES:
        for M in pc.M_CLASSES:
            yield f"mclass {F}x{K}x{M}", (lambda F=F, K=K, M=M: pc.route_case(F, K, M, 3)[:2]), 3
    for F, K, M, A in pc.LADDER_SHAPES:
        for cond in pc.LADDER_COND:
            yield f"ladder {F}x{K}x{M}x{A} cond {cond:.0e}", (lambda F=F, K=K, M=M, A=A, cond=cond: pc.route_case(F, K, M, A, cond=cond)[:2]), A
    for M in pc.GAP_M:
        yield f"gap M={M}", (lambda M=M: pc.gap_case(M)), pc.GAP_A
    yield "zero first entry", pc.zero_first_case, pc.ZERO_FIRST[2]


CASES = list(designed_cases())


@needs_longdouble
@pytest.mark.parametrize("name,make,A", CASES, ids=[c[0] for c in CASES])
def test_yardstick_of_every_designed_case(name, make, A):
    """Every component of every designed case can be gated: the float64 restatement is within 1e-13 of the
    longdouble one, in three orders of the variables (no component is left out on the GPU)."""
    XTX, XTY = make()
    n = min(XTX.shape[0], pc.DISTINCT)
    Y, worst_def = pc.case_yardstick(XTX[:n], XTY[:n], A)
    print(f"{name}: yardstick {Y.max():.2e}, oracle deficit {worst_def / pc.U:.1f} u")
    assert np.all(Y <= pc.YARDSTICK_CAP), (name, Y)
    assert np.all(Y > 0)


def test_zero_first_case_is_what_it_says():
    """The dominant eigenvector of XTY^T XTY has a first entry of exactly zero, the matrix is block diagonal to
    the bit, and the restated squaring finds the vector all the same (column of the LARGEST diagonal entry)."""
    _, XTY = pc.zero_first_case()
    for f in range(XTY.shape[0]):
        S = XTY[f].T @ XTY[f]
        assert np.all(S[0, 1:] == 0) and np.all(S[1:, 0] == 0) and S[0, 0] > 0
        assert S[0, 0] < 0.5 * np.linalg.eigvalsh(S)[-1]
        q = dominant_q_squaring(S)
        assert q[0] == 0.0 and abs(q @ q - 1) <= 4 * pc.U


def test_conditioning_ladder_is_what_it_says():
    for cond in pc.LADDER_COND:
        XTX, _ = pc.folds(1, 2, 32, 3, cond)
        c = np.linalg.cond(XTX[0])
        assert cond <= c <= 100 * cond, (cond, c)
        assert pc.same_bits(XTX[0], XTX[0].T.copy())


@pytest.mark.parametrize("M", [1, 2, 3, 5])
def test_exhaustion_fixture_is_exact(M):
    K, A, S, rows = 33, 5, 5, 7
    XTX, XTY, want = pc.exhaustion_case(8, K, M, A, S, rows)
    assert sorted(set(want["n_fit"])) == list(range(min(M, 3) + 1))
    for f in range(8):
        B, W, P, Q, R, n = ikpls_fit(XTX[f], XTY[f], A, eig="squaring")
        assert n == want["n_fit"][f]
        for got, key in ((B, "B"), (W, "W"), (P, "P"), (Q, "Q"), (R, "R")):
            assert np.array_equal(got, want[key][f]), (f, key)


@pytest.mark.parametrize("M", [1, 3])
def test_the_oracle_has_no_answer_for_a_non_finite_fold(M):
    """Why the GPU test states a contract instead of asking the oracle: on each non-finite fold ikpls_fit
    raises, or stops early and leaves zeros (a finite model that predicts the training mean)."""
    K, A = 33, 4
    XTX, XTY = pc.folds(5, 1, K, M)
    assert ikpls_fit(XTX[0], XTY[0], A)[5] == A
    for name, poke in pc.nonfinite_kinds(K, M, 5, 7):
        X, Y = XTX[0].copy(), XTY[0].copy()
        poke(X, Y)
        assert not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))), name
        try:
            with np.errstate(all="ignore"):
                B, *_, n = ikpls_fit(X, Y, A)
        except np.linalg.LinAlgError:
            continue
        assert n < A and np.all(B[n:] == 0), (name, n)


def test_route_table_is_what_the_planner_does():
    """Host logic (256 CUs without a device): every entry takes the route, slice count and XTX placement it
    is listed with.  Not marked gpu, but it asks the built library's planner: without libcvmhip.so
    (python -m cvmatrix_amd.build) it ends in the loader's ImportError."""
    for F, K, M, A, dtype, kernel, slices, in_lds in pc.ROUTES + [pc.ROUTE_F32]:
        pc.assert_plan(F, K, M, A, dtype, kernel, slices, in_lds)
    for F, K, kernel in pc.M_CLASS_ROUTES:
        for M in pc.M_CLASSES:
            pc.assert_plan(F, K, M, 3, np.float64, kernel)
    assert pc.plan(9, 33, 2, 6)["rows"] == 7 and pc.plan(2, 1028, 1, 4)["rows"] == 9
