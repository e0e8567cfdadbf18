"""GPU (-m gpu): the device elastic net / lasso (cvm_enet_fit, cvmatrix_amd/enet.py) against the two derived
gates of tests/enet_cases.py -- the KKT certificate evaluated in extended precision, and the strong-convexity
distance to the NumPy reference -- and its contract: penalty order, lambda >= lambda_max, the ridge limit, the
status codes, bit-reproducibility whatever the workspace, and the pipeline end to end.

Where the kernel lands on the MI355X (each test prints it): gate 1 at most 0.50 of its bound in float64 and 0.98
in float32 (there the bound is the rounding of the store itself), gate 2 at most 0.98 (rho = 0.05, where the
Hessian is nearly mu I and the inequality nearly an equality); sweeps at most 394 (K = 3, rho = 1; the reference from zero: 379).

The conditions these tests rest on (the reference converges well inside max_sweeps, mu > 0, the support of every
grid case is decided at the device's tolerance) are asserted on the CPU in tests/test_enet_host.py."""

import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import enet_cases as ec

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import enet as mod
    return mod


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the fixtures are read-only)


def fit_np(emod, XTX, XTY, lams, rho, dtype=np.float64, **kw):
    fit = emod.enet_fit_batched(dev(XTX, dtype), dev(XTY, dtype), lams, rho, **kw)
    assert fit.B.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    return fit.B.cpu().numpy(), fit.info.cpu().numpy(), fit.sweeps.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_case(emod, XTX, XTY, lams, rho, ref, dtype, what, count=True):
    F, K, M = XTY.shape
    B, info, sweeps = fit_np(emod, XTX, XTY, lams, rho, dtype, tol=ec.GPU_TOL, max_sweeps=ec.MAX_SWEEPS)
    assert B.shape == (F, len(lams), K, M) and info.shape == sweeps.shape == (F, len(lams), M)
    print(f"{what}: sweeps at most {sweeps.max()}, nonzeros at most {(B != 0).sum(axis=2).max()}")
    assert np.all(info == 0), (what, np.argwhere(info != 0)[:5])
    assert np.all(sweeps >= 1) and np.all(sweeps <= ec.MAX_SWEEPS)
    n = ec.assert_gates(XTX, XTY, lams, rho, ec.GPU_TOL, B, info, ref, float32=dtype == np.float32, what=what)
    assert n == F * len(lams) * M
    if count:
        assert np.array_equal((B != 0).sum(axis=2), (ref != 0).sum(axis=2)), what
    return B


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("rho", ec.GRID_RHO)
@pytest.mark.parametrize("M", ec.GRID_M)
@pytest.mark.parametrize("K", ec.GRID_K)
def test_shape_grid(emod, K, M, rho, dtype):
    """K at the lane-count edges of a 64-wide wave and over one and several 256-coordinate passes, M on both
    sides of a fold's share of an XCD, rho = 1 (sparse: the active set), 0.5 and 0.05 (up to 200 nonzeros: the
    fallback): both gates and the number of nonzeros for all F x L x M problems."""
    XTX, XTY, lams, ref = ec.grid_case(K, M, rho)
    check_case(emod, XTX, XTY, lams, rho, ref, dtype, f"grid K={K} M={M} rho={rho} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", list(ec.ROUTE_CASES))
def test_route_boundaries(emod, name, dtype):
    """A dense solution that fills the 64 active slots exactly (K = 64) and one that overflows them into the
    fallback (K = 65, every coefficient nonzero); the fallback on each side of the LDS layout change at K = 2048."""
    XTX, XTY, lams, rho, ref, dense = ec.route_case(name)
    B = check_case(emod, XTX, XTY, lams, rho, ref, dtype, f"{name} {np.dtype(dtype).name}", count=dense)
    if dense:
        assert np.all(B[0, -1] != 0)
    else:
        assert (B[0, -1] != 0).sum() > 64            # more than the active set holds: the fallback ran


def test_penalty_order(emod):
    """The penalties in shuffled order: the bits of the sorted call, permuted (info and sweeps with them)."""
    XTX, XTY, lams, _ = ec.grid_case(65, 3, 0.5)
    lams = np.concatenate([lams, [1.5 * lams[0], 0.3 * lams[0]]])
    srt = np.sort(lams)[::-1]
    B0, i0, s0 = fit_np(emod, XTX, XTY, srt, 0.5)
    assert np.all(i0 == 0)
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(lams.size)
        B, info, sweeps = fit_np(emod, XTX, XTY, srt[perm], 0.5)
        assert same_bits(B, B0[:, perm]) and same_bits(info, i0[:, perm]) and same_bits(sweeps, s0[:, perm])
    B, info, sweeps = fit_np(emod, XTX, XTY, srt[::-1].copy(), 0.5)
    assert same_bits(B, B0[:, ::-1])


@pytest.mark.parametrize("rho", [1.0, 0.25])
def test_at_or_above_lambda_max(emod, rho):
    XTX, XTY, _, _ = ec.grid_case(63, 3, 1.0)
    A, Y = dev(XTX), dev(XTY)
    lmax = emod.lambda_max(Y, rho)
    assert lmax.shape == (3, 3) and same_bits(lmax.cpu().numpy(), ec.lambda_max(XTY, rho))
    top = float(lmax.max())
    fit = emod.enet_fit_batched(A, Y, [top, 3.0 * top, 1e300], rho, check=True)
    assert torch.count_nonzero(fit.B) == 0
    assert torch.all(fit.info == 0) and torch.all(fit.sweeps == 1)
    # each problem at its own lambda_max exactly, and just below it
    lm = lmax.cpu().numpy()
    for f in range(3):
        for m in range(3):
            fit = emod.enet_fit_batched(A[f], Y[f, :, m], [lm[f, m], lm[f, m] * (1 - 1e-6)], rho, check=True)
            assert torch.count_nonzero(fit.B[0, 0]) == 0 and int(fit.sweeps[0, 0, 0]) == 1
            assert torch.count_nonzero(fit.B[0, 1]) >= 1 and int(fit.sweeps[0, 1, 0]) > 1
    grid = emod.lambda_grid(Y, rho)
    assert grid.shape == (20,) and grid[0] == top and abs(grid[-1] / top - 1e-3) < 1e-15


def test_ridge_limit(emod):
    """rho -> 0: the ridge solution b_r at lambda (1 - rho) has a subgradient of the elastic net objective of norm
    at most |h - (G + lambda (1 - rho) I) b_r|_2 + lambda rho sqrt(K), so by strong convexity
    |b - b_r|_2 <= (|v(b)|_2 + that) / mu."""
    from cvmatrix_amd.ridge import ridge_fit_batched
    rho = 1e-6
    K, M = 65, 3
    XTX, XTY, lams, _ = ec.grid_case(K, M, 0.05)
    B, info, _ = fit_np(emod, XTX, XTY, lams, rho, tol=ec.GPU_TOL)
    Br = ridge_fit_batched(dev(XTX), dev(XTY), lams * (1 - rho)).B.cpu().numpy()
    assert np.all(info == 0)
    for f in range(3):
        lmin = float(np.linalg.eigvalsh(XTX[f])[0])
        for l, lam in enumerate(lams):
            mu = lmin + lam * (1 - rho)
            for m in range(M):
                G, h = XTX[f], XTY[f][:, m]
                res = np.linalg.norm(h - G @ Br[f, l, :, m] - lam * (1 - rho) * Br[f, l, :, m])
                bound = (np.linalg.norm(ec.kkt_violation(G, h, B[f, l, :, m], lam, rho)) + res + lam * rho * np.sqrt(K)) / mu
                d = np.linalg.norm(B[f, l, :, m] - Br[f, l, :, m])
                assert d <= bound, (f, l, m, d, bound)
                assert d <= 1e-3 * np.linalg.norm(Br[f, l, :, m])          # (and the bound says something)


def cond_1e4_design(M=2):
    n, K, cond = ec.DESIGNS[1]
    return ec.fold_matrices(n, K, cond, M, 1, seed=7, f32_exact=False)


def test_status_max_sweeps(emod):
    """max_sweeps = 2 at 0.01 lambda_max of the cond-1e4 design (the reference needs >= 20 sweeps there:
    tests/test_enet_host.py): info 1, sweeps == 2, B finite; the penalty above lambda_max in the same call
    converges and passes the gate."""
    XTX, XTY = cond_1e4_design()
    rho = 0.5
    top = ec.lambda_max(XTY, rho).max()
    lams = np.array([0.01 * top, 2.0 * top])
    B, info, sweeps = fit_np(emod, XTX, XTY, lams, rho, max_sweeps=2)
    assert np.all(info[:, 0] == 1) and np.all(sweeps[:, 0] == 2) and np.all(np.isfinite(B[:, 0]))
    assert np.any(B[:, 0] != 0)
    assert np.all(info[:, 1] == 0) and np.all(sweeps[:, 1] == 1)
    ref = np.zeros_like(B)
    assert ec.assert_gates(XTX, XTY, lams, rho, 1e-8, B, info, ref, what="beside status 1") == 2
    with pytest.warns(emod.EnetConvergenceWarning, match=r"fold 0, lambda\[0\].*response 0"):
        emod.enet_fit_batched(dev(XTX), dev(XTY), lams, rho, max_sweeps=2, check=True)
    assert issubclass(emod.EnetConvergenceWarning, RuntimeWarning)
    with warnings.catch_warnings():
        warnings.simplefilter("error", emod.EnetConvergenceWarning)
        emod.enet_fit_batched(dev(XTX), dev(XTY), lams, rho, check=True)          # converges: no warning


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_status_not_finite(emod, dtype):
    """NaN in one response's column of XTY (fold 1, response 1) and on the diagonal of one fold's XTX (fold 2):
    info 2 and NaN exactly there; every other problem passes both gates."""
    K, M, rho = 65, 3, 0.5
    XTX, XTY, lams, ref = ec.grid_case(K, M, rho)
    XTX, XTY = XTX.copy(), XTY.copy()
    XTY[1, 40, 1] = np.nan
    XTX[2, 7, 7] = np.nan
    B, info, sweeps = fit_np(emod, XTX, XTY, lams, rho, dtype, tol=ec.GPU_TOL)
    want = np.zeros(info.shape, bool)
    want[1, :, 1] = True
    want[2] = True
    assert np.array_equal(info == 2, want) and np.all(info[~want] == 0), info
    nanB = np.isnan(B).all(axis=2)
    assert np.array_equal(nanB, want) and np.array_equal(np.isnan(B).any(axis=2), want)
    clean_XTX, clean_XTY, _, _ = ec.grid_case(K, M, rho)
    n = ec.assert_gates(clean_XTX, clean_XTY, lams, rho, ec.GPU_TOL, np.where(np.isnan(B), 0.0, B), info, ref,
                        float32=dtype == np.float32, what="beside status 2", only=~want)
    assert n == (~want).sum()
    with pytest.raises(np.linalg.LinAlgError, match="fold 1.*response 1"):
        emod.enet_fit_batched(dev(XTX, dtype), dev(XTY, dtype), lams, rho, check=True)
    # an infinity in h
    XTX, XTY = clean_XTX.copy(), clean_XTY.copy()
    XTY[0, 3, 0] = np.inf
    B, info, _ = fit_np(emod, XTX, XTY, lams, rho, dtype)
    assert np.all(info[0, :, 0] == 2) and np.all(np.isnan(B[0, :, :, 0])) and np.all(info[0, :, 1:] == 0)
    assert np.all(info[1:] == 0) and np.all(np.isfinite(B[1:]))


def test_zero_column_stays_at_zero(emod):
    """G_jj = 0 with rho = 1: the denominator is not > 0 and the coordinate stays at zero (scikit-learn's rule
    for a zero column); the problem converges and passes gate 1."""
    K, M, rho = 33, 2, 1.0
    n = 120
    X, Y = ec.design(n, K, 10.0, M, seed=3)
    X[:, 5] = 0.0
    X[:, 32] = 0.0
    XTX, XTY = (X.T @ X)[None], (X.T @ Y)[None]
    XTX = 0.5 * (XTX + XTX.transpose(0, 2, 1))
    lams = np.array([0.3, 0.01]) * ec.lambda_max(XTY, rho).max()
    B, info, _ = fit_np(emod, XTX, XTY, lams, rho, tol=ec.GPU_TOL)
    assert np.all(info == 0) and np.all(B[:, :, [5, 32]] == 0) and np.all((B != 0).sum(axis=2) >= 1)
    for l, lam in enumerate(lams):
        for m in range(M):
            v = ec.kkt_violation(XTX[0], XTY[0][:, m], B[0, l, :, m], lam, rho)
            assert np.all(v <= ec.first_gate_bound(XTX[0], XTY[0][:, m], B[0, l, :, m], lam, rho, ec.GPU_TOL))


def cabi_fit(XTX, XTY, lams, rho, tol, max_sweeps, paths=None):
    """cvm_enet_fit through the C ABI with a workspace of `paths` slots (None: what the library asks for)."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = XTY.shape
    lams = np.ascontiguousarray(lams, dtype=np.float64)
    L = lams.size
    one = lib.cvm_enet_workspace_bytes(1, K, 1, 1)
    nbytes = lib.cvm_enet_workspace_bytes(F, K, M, L) if paths is None else paths * one
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    B = torch.full((F, L, K, M), -7.0, dtype=XTX.dtype, device="cuda")
    info = torch.full((F, L, M), -7, dtype=torch.int32, device="cuda")
    sweeps = torch.full((F, L, M), -7, dtype=torch.int32, device="cuda")
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_enet_fit(XTX.data_ptr(), XTY.data_ptr(), F, K, M, lams.ctypes.data, L, rho, tol, max_sweeps, code,
                          B.data_ptr(), info.data_ptr(), sweeps.data_ptr(), ws.data_ptr(), nbytes,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cvm_last_error()
    torch.cuda.synchronize()
    return B, info, sweeps


def test_reproducible_whatever_the_workspace(emod):
    """Two runs are bit-equal; F = 11 folds x 3 responses through workspaces of one path, of five and of all 33
    give the same bits (ws_bytes handed to the C entry); less than one path is CVM_EWORKSPACE."""
    from cvmatrix_amd import _lib
    K, M, F, rho = 65, 3, 11, 0.5
    XTX, XTY = ec.fold_matrices(2 * K + 40, K, ec.GRID_COND, M, F, seed=11)
    lams = ec.GRID_FRACTIONS * ec.lambda_max(XTY, rho).max()
    A, Y = dev(XTX), dev(XTY)
    first = emod.enet_fit_batched(A, Y, lams, rho)
    again = emod.enet_fit_batched(A, Y, lams, rho)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert torch.all(first.info == 0)
    for paths in (1, 5, None):
        B, info, sweeps = cabi_fit(A, Y, lams, rho, 1e-8, 1000, paths)
        assert torch.equal(B, first.B) and torch.equal(info, first.info) and torch.equal(sweeps, first.sweeps), paths
    # one fold alone has the bits it has in the batch
    alone = emod.enet_fit_batched(A[4], Y[4], lams, rho)
    assert torch.equal(alone.B[0], first.B[4]) and torch.equal(alone.sweeps[0], first.sweeps[4])
    lib = _lib.load()
    one = lib.cvm_enet_workspace_bytes(1, K, 1, 1)
    ws = torch.empty(one, dtype=torch.uint8, device="cuda")
    lam_c = np.ascontiguousarray(lams)
    args = (A.data_ptr(), Y.data_ptr(), F, K, M, lam_c.ctypes.data, lams.size)
    outs = (_lib.CVM_F64, first.B.data_ptr(), first.info.data_ptr(), first.sweeps.data_ptr(), ws.data_ptr())
    assert lib.cvm_enet_fit(*args, rho, 1e-8, 1000, *outs, one - 1, None) == _lib.CVM_EWORKSPACE
    for bad, text in (((0.0, 1e-8, 1000), b"l1_ratio"), ((1.5, 1e-8, 1000), b"l1_ratio"), ((0.5, 1e-13, 1000), b"tol"),
                      ((0.5, 1.0, 1000), b"tol"), ((0.5, 1e-8, 0), b"max_sweeps")):
        assert lib.cvm_enet_fit(*args, *bad, *outs, one, None) == _lib.CVM_EINVAL
        assert text in lib.cvm_last_error()
    lam_bad = np.array([1.0, 0.0])
    assert lib.cvm_enet_fit(A.data_ptr(), Y.data_ptr(), F, K, M, lam_bad.ctypes.data, 2, rho, 1e-8, 1000, *outs, one,
                            None) == _lib.CVM_EINVAL
    assert b"> 0" in lib.cvm_last_error()
    torch.cuda.synchronize()


def test_limit_shapes(emod):
    """F = 0 launches nothing; a single (K, K) with (K,) is one fold with one response; lasso_fit_batched is
    l1_ratio = 1."""
    K, M = 33, 2
    XTX, XTY = ec.fold_matrices(2 * K + 40, K, ec.GRID_COND, M, 2, seed=5)
    A, Y = dev(XTX), dev(XTY)
    lams = np.array([0.3, 0.05]) * ec.lambda_max(XTY, 1.0).max()
    empty = emod.enet_fit_batched(A[:0], Y[:0], lams, check=True)
    assert empty.B.shape == (0, 2, K, M) and empty.info.shape == empty.sweeps.shape == (0, 2, M)
    assert empty.B.dtype == torch.float64 and empty.info.dtype == torch.int32
    ref = emod.enet_fit_batched(A, Y, lams, 1.0)
    one = emod.lasso_fit_batched(A[1], Y[1, :, 1], lams, check=True)
    assert one.B.shape == (1, 2, K, 1) and one.info.shape == (1, 2, 1)
    assert torch.equal(one.B[0, :, :, 0], ref.B[1, :, :, 1]) and torch.equal(one.sweeps[0, :, 0], ref.sweeps[1, :, 1])


@pytest.mark.parametrize("rho", [1.0, 0.5])
def test_end_to_end(emod, rho):
    """CVMatrix -> training_XTX_XTY_batched -> enet_fit_batched -> pls_validation_sse and cv_predict at N = 240,
    K = 12, M = 2, 4 folds, against the same pipeline in NumPy with the reference solver (both at tol = 1e-12).
    The designs have cond(XTX) of order 10 and mu of the order of max|h|, so the two solutions differ by about
    1e-11 relative: predictions and per-lambda SSE to 1e-9 relative, the tolerance of the ridge and PCR
    end-to-end tests."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import pls_validation_sse
    from cvmatrix_amd.predict import cv_predict
    rng = np.random.default_rng(17)
    N, K, M, P = 240, 12, 2, 4
    X = rng.standard_normal((N, K)) + 0.5
    beta = np.zeros((K, M))
    beta[[1, 4, 7], 0] = [2.0, -1.5, 1.0]
    beta[[0, 4, 9, 11], 1] = [1.0, 1.0, -2.0, 0.5]
    Y = X @ beta + 0.3 * rng.standard_normal((N, M)) + 1.0
    labels = rng.integers(0, P, N)
    folds = [np.flatnonzero(labels == f) for f in range(P)]
    cvm = amd.CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    lams = emod.lambda_grid(XTY, rho, n=6, eps=1e-2)
    fit = emod.enet_fit_batched(XTX, XTY, lams, rho, tol=1e-12, check=True)
    sse, wsum = pls_validation_sse(cvm, batch, stats, fit.B)
    pred = cv_predict(cvm, batch, stats, fit.B).cpu().numpy()          # (N, L, M)
    ref_pred, ref_sse = ec.numpy_pipeline(X, Y, folds, lams, rho)
    nnz = (fit.B != 0).sum(dim=2).cpu().numpy()
    assert nnz.min() <= 2 and nnz.max() >= 6                             # the grid runs from sparse to dense
    assert np.abs(pred.transpose(1, 0, 2) - ref_pred).max() <= 1e-9 * np.abs(ref_pred).max()
    np.testing.assert_allclose(sse.cpu().numpy(), ref_sse, rtol=1e-9)
    assert np.array_equal(wsum.cpu().numpy(), [len(v) for v in folds])


def test_example_against_sklearn(emod):
    """examples/fast_cv_enet.py: cross-validated RMSE per penalty against scikit-learn's ElasticNet refitted on every
    training set (alpha = lambda / n_train, fit_intercept=True).  scikit-learn stops on a duality gap of
    1e-12 |y|^2, which by strong convexity (mu about n / 2 here) bounds its coefficients' error by
    sqrt(2 gap / mu), about 1e-6 of their size; the device runs at tol = 1e-10 and is far inside that: RMSE to 1e-6."""
    pytest.importorskip("sklearn.linear_model")
    spec = importlib.util.spec_from_file_location("fast_cv_enet", os.path.join(ROOT, "examples", "fast_cv_enet.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(5)
    N, K, M, P = 400, 12, 2, 5
    X = rng.standard_normal((N, K))
    beta = np.zeros((K, M))
    beta[[0, 3, 8], 0] = [1.5, -1.0, 0.5]
    beta[[2, 3], 1] = [1.0, 2.0]
    Y = X @ beta + 0.5 * rng.standard_normal((N, M)) + 2.0
    labels = np.arange(N) % P
    for rho in (1.0, 0.5):
        lambdas, rmse, nonzeros = ex.fast_cv_rmse(X, Y, labels, rho, n_lambdas=6, eps=1e-2, tol=1e-10)
        assert lambdas.shape == (6,) and rmse.shape == nonzeros.shape == (6, M) and nonzeros[0].max() <= 1
        ref = ex.sklearn_cv_rmse(X, Y, labels, rho, lambdas)
        np.testing.assert_allclose(rmse, ref, rtol=1e-6)
