"""CPU: the ridge oracle (oracle/ridge_oracle.py) against its own pins -- mpmath at 50 digits,
scikit-learn, LAPACK's dpotrf, each where importable -- and every fixture generator of
tests/ridge_cases.py against the conditions the GPU tests rely on (the reference converges, the failing
pivot is unambiguous, the shape grid covers what it says)."""

import numpy as np
import pytest

import ridge_cases as rc
from oracle import ridge_oracle as ro

needs_longdouble = pytest.mark.skipif(not ro.LONGDOUBLE_OK, reason=ro.LONGDOUBLE_REASON)
U = ro.U


@needs_longdouble
@pytest.mark.parametrize("K,M,cond,lam", [(5, 2, 1e4, 0.0), (33, 3, 1e8, 0.0), (64, 2, 1e12, 0.0), (40, 3, 1e12, 1e-9),
                                          (64, 1, 1e8, 1e-3), (1, 1, 1e4, 0.5), (2, 3, 1e12, 0.0)])
def test_reference_against_mpmath(K, M, cond, lam):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rng = np.random.default_rng(K + M)
    XTX, XTY = rc.spd_spectrum(rng, 1, K, M, cond)
    A = mp.matrix(XTX[0].tolist()) + mp.mpf(lam) * mp.eye(K)
    cols = [mp.lu_solve(A, mp.matrix(XTY[0][:, j].tolist())) for j in range(M)]
    exact = np.array([[float(cols[j][i]) for j in range(M)] for i in range(K)])
    got = ro.ridge_solve_ref(XTX[0], XTY[0], lam)
    assert ro.rel_err(got, exact) <= 4 * U
    # element by element too: the float64 nearest the exact value, give or take one unit in the last place
    assert np.all(np.abs(got - exact) <= np.spacing(np.abs(exact)))


@needs_longdouble
def test_reference_against_sklearn():
    lm = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((200, 12)), rng.standard_normal((200, 3))
    for alpha in (0.01, 1.0, 50.0):
        ref = lm.Ridge(alpha=alpha, fit_intercept=False, solver="cholesky").fit(X, Y).coef_.T
        assert ro.rel_err(ro.ridge_solve_ref(X.T @ X, X.T @ Y, alpha), ref) <= 1e-12


@needs_longdouble
def test_reference_vector_and_failures():
    rng = np.random.default_rng(4)
    XTX, XTY = rc.spd_spectrum(rng, 1, 20, 1, 1e3)
    assert np.array_equal(ro.ridge_solve_ref(XTX[0], XTY[0, :, 0], 0.1), ro.ridge_solve_ref(XTX[0], XTY[0], 0.1)[:, 0])
    bad = rc.make_indefinite(XTX[0].copy(), 7)
    with pytest.raises(np.linalg.LinAlgError):
        ro.ridge_solve_ref(bad, XTY[0], 0.0)
    # singular to working precision: no fixture
    with pytest.raises(np.linalg.LinAlgError):
        ro.ridge_solve_ref(rc.spd_spectrum(rng, 1, 30, 2, 1e17)[0][0], rng.standard_normal((30, 2)), 0.0)


@pytest.mark.parametrize("K", rc.INFO_K)
def test_cholesky_info_on_the_indefinite_fixtures(K):
    """The fixtures of the GPU test (d): the oracle names pivot j, with a value below -1e-3 ||A||_2, at both
    penalties of that test; LAPACK agrees where scipy is importable."""
    for j in rc.info_pivots(K):
        XTX, _ = rc.indefinite_fixture(K, j)
        for lam in (0.0, 1e-3):
            A = XTX[1] + lam * np.eye(K)
            info, piv = ro.cholesky_info(A)
            assert info == j and piv < -1e-3 * np.linalg.norm(A, 2), (K, j, lam, info, piv)
            assert rc.info_is_unambiguous(A, info, piv)
            for f in (0, 2, 3):
                i0, p0 = ro.cholesky_info(XTX[f] + lam * np.eye(K))
                assert i0 == 0 and rc.info_is_unambiguous(XTX[f], i0, p0)
    lapack = pytest.importorskip("scipy.linalg.lapack")
    for j in rc.info_pivots(K):
        XTX, _ = rc.indefinite_fixture(K, j)
        assert lapack.dpotrf(XTX[1], lower=1)[1] == j
        assert lapack.dpotrf(XTX[0], lower=1)[1] == 0


def test_cholesky_info_on_non_finite_input():
    rng = np.random.default_rng(6)
    A = rc.spd_spectrum(rng, 1, 40, 1, 1e2)[0][0]
    for j in (1, 17, 33, 40):
        B = A.copy(); B[j - 1, j - 1] = np.nan
        assert ro.cholesky_info(B)[0] == j
        B = A.copy(); B[j - 1, j - 1] = np.inf
        assert ro.cholesky_info(B) == (j, np.inf)
    B = A.copy(); B[35, 4] = B[4, 35] = np.nan
    assert ro.cholesky_info(B)[0] == 36
    info, piv = ro.cholesky_info(A)
    assert info == 0 and 0.5e-2 <= piv <= 1.0
    assert ro.cholesky_info(np.array([[-1.0]])) == (1, -1.0)


def test_grid_covers_what_it_says():
    assert len(rc.GRID) >= 48 and len(set(rc.GRID)) == len(rc.GRID)
    assert {k for k, _ in rc.GRID} == set(rc.K_VALUES) and {m for _, m in rc.GRID} == set(rc.M_VALUES)
    for grid, least in ((rc.GRID, 3), (rc.GRID_F32, 2)):
        for cls in (0, 1, 31):
            hit = [(k, m) for k, m in grid if (k + m) % 32 == cls]
            assert len(hit) >= least, (cls, hit)
            assert any(k % 32 == 0 for k, _ in hit) and any(k % 32 for k, _ in hit), (cls, hit)
    assert len(rc.GRID_F32) == 16 and set(rc.GRID_F32) <= set(rc.GRID)
    assert {(m + 15) // 16 for _, m in rc.GRID_F32} == {1, 2, 3, 4}


@needs_longdouble
def test_grid_and_ladder_fixtures_converge():
    """The references of the ladder (float64 to cond 1e12, float32 to 1e6; every K, three of the six (K, M):
    the GPU test raises where one of the others does not converge) and a sample of the grid: the refinement
    converges and the prescribed spectrum is there."""
    for K, M in rc.LADDER_KM[1::2][:2] + rc.LADDER_KM[4:5]:
        for cond in rc.LADDER_COND:
            rng = np.random.default_rng(int(K * 100 + M + np.log10(cond)))
            XTX, XTY = rc.spd_spectrum(rng, 1, K, M, cond)
            assert abs(np.log10(np.linalg.cond(XTX[0]) / cond)) < 0.01 or cond > 1e11
            for lv in rc.ladder_lambdas(cond):
                ro.ridge_solve_ref(XTX[0], XTY[0], lv)
        for cond in rc.LADDER_COND_F32:
            rng = np.random.default_rng(K + M)
            XTX, XTY = rc.spd_spectrum(rng, 1, K, M, cond, np.float32)
            assert XTX.dtype == np.float32 and np.array_equal(XTX[0], XTX[0].T)
            for lv in rc.ladder_lambdas(cond):
                info, piv = ro.cholesky_info(XTX[0].astype(np.float64) + lv * np.eye(K))
                assert info == 0
                ro.ridge_solve_ref(XTX[0], XTY[0], lv)
    for K, M in rc.GRID[::7]:
        XTX, XTY = rc.spd_spectrum(np.random.default_rng(K), 1, K, M, 1e2)
        ref, Y = rc.references(XTX, XTY, [0.0, 1e-4, 10.0])
        assert np.all(Y < 1e-12)


@needs_longdouble
def test_gate_helper():
    rng = np.random.default_rng(12)
    XTX, XTY = rc.spd_spectrum(rng, 3, 20, 2, 1e6)
    lam = [0.0, 1e-3]
    ref, Y = rc.references(XTX, XTY, lam)
    assert Y[0] > Y[1] > 0
    assert rc.assert_gate(ref, ref, Y, "exact") == 0.0
    lapack = np.array([[np.linalg.solve(XTX[f] + lv * np.eye(20), XTY[f]) for lv in lam] for f in range(3)])
    assert rc.assert_gate(lapack, ref, Y, "lapack") <= 1.0
    with pytest.raises(AssertionError):
        rc.assert_gate(ref * (1 + 1e-9), ref, Y, "off")
    swapped = ref[[1, 0, 2]]
    with pytest.raises(AssertionError):
        rc.assert_gate(swapped, ref, Y, "swapped folds")
    r32 = ref.astype(np.float32)
    rc.assert_gate(r32, ref, Y, "rounded once", float32=True)
    with pytest.raises(AssertionError):
        rc.assert_gate(r32, ref, Y, "float32 through the float64 gate")


def test_random_draws_can_be_called_by_the_oracle():
    """Test (j)'s generator: the oracle alone can call `info` in at least nine draws of ten, every
    indefinite fold fails at every penalty, and the draws cover both dtypes and all four response tiles."""
    left_out, dtypes, tiles, bad = 0, set(), set(), 0
    n = 0
    for d in rc.random_draws():
        n += 1
        info, sure = rc.oracle_info(d["XTX"], d["lam"])
        left_out += not sure.all()
        dtypes.add(d["dtype"])
        tiles.add((d["M"] + 15) // 16)
        if d["bad_fold"] is not None:
            bad += 1
            assert np.all(info[d["bad_fold"]] > 0) and np.all(info[d["bad_fold"]] == info[d["bad_fold"], 0])
            assert np.all(np.delete(info, d["bad_fold"], axis=0) == 0)
        else:
            assert np.all(info == 0)
    assert n == rc.RANDOM_DRAWS == 150 and bad == 15
    assert left_out * 10 <= n, left_out
    assert dtypes == {np.float32, np.float64} and tiles == {1, 2, 3, 4}
