"""CPU: the host half of the device elastic net -- the argument rules of cvmatrix_amd/enet.py before any
device is touched, the workspace sizing through the C ABI, lambda_max / lambda_grid on host tensors -- and the
conditions the GPU tests (tests/test_gpu_enet.py) rest on: the NumPy reference solver of tests/enet_cases.py
against scikit-learn, the two gates on the reference itself, and what is asserted of the designs."""

import warnings

import numpy as np
import pytest
import torch

import enet_cases as ec
from cvmatrix_amd import _lib
from cvmatrix_amd import enet


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


A3 = torch.eye(3, dtype=torch.float64)
Y3 = torch.ones((3, 1), dtype=torch.float64)


@pytest.mark.parametrize("bad", [[0.0], [-1.0], [0.5, np.nan], [np.inf], [], np.ones(257), np.ones((2, 2)), [[1.0]]])
def test_penalty_grid_is_refused(bad):
    with pytest.raises(ValueError):
        enet.check_lambdas(bad)
    with pytest.raises(ValueError):
        enet.enet_fit_batched(A3, Y3, bad)


def test_penalty_grid_is_accepted():
    lam = enet.check_lambdas([3, 1e-300, 1e300])
    assert lam.dtype == np.float64 and lam.flags.c_contiguous and lam.tolist() == [3.0, 1e-300, 1e300]
    assert enet.check_lambdas(np.ones(256)).size == 256


@pytest.mark.parametrize("kwargs", [{"l1_ratio": 0.0}, {"l1_ratio": -0.1}, {"l1_ratio": 1.0000001}, {"l1_ratio": np.nan},
                                    {"tol": 0.9e-12}, {"tol": 1.0}, {"tol": np.nan}, {"max_sweeps": 0},
                                    {"max_sweeps": 2.5}])
def test_solver_arguments_are_refused(kwargs):
    with pytest.raises(ValueError):
        enet.enet_fit_batched(A3, Y3, [1.0], **kwargs)


def test_l1_ratio_zero_points_to_ridge():
    with pytest.raises(ValueError, match="ridge_fit_batched"):
        enet.enet_fit_batched(A3, Y3, [1.0], 0.0)
    with pytest.raises(TypeError):
        enet.lasso_fit_batched(A3, Y3, [1.0], l1_ratio=0.5)          # the lasso has no mixing value


def test_solver_arguments_are_accepted():
    assert enet.check_solver_arguments(1, 1e-12, 1) == (1.0, 1e-12, 1)
    assert enet.check_solver_arguments(1e-6, 0.5, np.int64(7)) == (1e-6, 0.5, 7)


def test_host_tensors_are_refused_before_the_device():
    with pytest.raises(TypeError):
        enet.enet_fit_batched(A3, Y3, [1.0])
    with pytest.raises(TypeError):
        enet.lasso_fit_batched(np.eye(3), np.ones((3, 1)), [1.0])


def test_workspace_bytes_is_host_arithmetic(lib):
    ws = lib.cvm_enet_workspace_bytes
    for K in (1, 31, 32, 33, 512, 2048, 2049, 4096):
        one = ws(1, K, 1, 1)
        assert one == (8 * K + 255) // 256 * 256
        for F, M, L in ((1, 1, 1), (3, 17, 5), (10, 16, 20), (100, 16, 20), (16, 64, 1), (17, 64, 256)):
            assert ws(F, K, M, L) == min(F * M, 1024) * one, (K, F, M, L)
    assert ws(0, 8, 1, 1) == ws(1, 8, 1, 1)
    assert ws(1, 0, 1, 1) == 0 and ws(1, 4097, 1, 1) == 0 and ws(1, 8, 65, 1) == 0 and ws(1, 8, 0, 1) == 0
    assert ws(1, 8, 1, 0) == 0 and ws(1, 8, 1, 257) == 0 and ws(-1, 8, 1, 1) == 0


def test_lambda_max_and_grid_on_host_tensors():
    rng = np.random.default_rng(0)
    H = rng.standard_normal((4, 9, 3))
    for rho in (1.0, 0.25):
        got = enet.lambda_max(torch.from_numpy(H), rho)
        assert got.shape == (4, 3)
        np.testing.assert_array_equal(got.numpy(), ec.lambda_max(H, rho))
        grid = enet.lambda_grid(torch.from_numpy(H), rho, n=7, eps=1e-2)
        assert grid.dtype == np.float64 and grid.shape == (7,) and np.all(np.diff(grid) < 0)
        assert grid[0] == np.abs(H).max() / rho
        np.testing.assert_allclose(grid[-1], 1e-2 * grid[0], rtol=1e-14)
        np.testing.assert_allclose(grid[1:] / grid[:-1], 1e-2 ** (1 / 6), rtol=1e-13)
    assert enet.lambda_max(torch.from_numpy(H[0]), 1.0).shape == (1, 3)
    assert enet.lambda_max(torch.from_numpy(H[0, :, 0]), 1.0).shape == (1, 1)
    assert enet.lambda_grid(torch.from_numpy(H), 1.0).shape == (20,)
    assert enet.lambda_grid(torch.from_numpy(H), 1.0, n=1).tolist() == [np.abs(H).max()]
    for bad in ({"n": 0}, {"n": 257}, {"eps": 0.0}, {"eps": 1.0}):
        with pytest.raises(ValueError):
            enet.lambda_grid(torch.from_numpy(H), 1.0, **bad)
    with pytest.raises(ValueError):
        enet.lambda_max(torch.from_numpy(H), 0.0)
    with pytest.raises(ValueError):
        enet.lambda_grid(torch.zeros((2, 3, 1), dtype=torch.float64), 1.0)


def issue_design(i, M=1):
    n, K, cond = ec.DESIGNS[i]
    XTX, XTY = ec.fold_matrices(n, K, cond, M, 1, seed=7, f32_exact=False)   # (cond 1e6: float32 would lose mu > 0)
    return n, XTX[0], XTY[0]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_reference_against_sklearn(i):
    """alpha = lambda / n, fit_intercept=False on the centred design: the supports agree, the coefficients
    within the distance bound of the two solutions' own violations."""
    lm = pytest.importorskip("sklearn.linear_model")
    n, K, cond = ec.DESIGNS[i]
    X, Y = ec.design(n, K, cond, 1, seed=7)
    G, H = X.T @ X, X.T @ Y
    G = 0.5 * (G + G.T)
    for rho in ec.DESIGN_RHO:
        lams = np.array(ec.DESIGN_FRACTIONS[:3]) * ec.lambda_max(H, rho).max()
        B, _, conv = ec.reference_path(G, H, lams, rho, tol=1e-12)
        assert conv.all()
        for l, lam in enumerate(lams):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sk = lm.ElasticNet(alpha=lam / n, l1_ratio=rho, fit_intercept=False, tol=1e-14, max_iter=200000,
                                   precompute=False).fit(X, Y[:, 0]).coef_
            d = np.linalg.norm(B[l, :, 0] - sk)
            assert d <= ec.distance_bound(G, H[:, 0], sk, B[l, :, 0], lam, rho), (i, rho, l, d)
            assert np.array_equal(sk != 0, B[l, :, 0] != 0), (i, rho, l)


@pytest.mark.parametrize("i", range(len(ec.DESIGNS)))
def test_the_gates_hold_on_the_reference_itself(i):
    """The NumPy rule at tol = 1e-10 against the NumPy rule at tol = 1e-12 on the four designs, rho in {1, 0.5},
    lambda / lambda_max in {0.5, 0.1, 0.01, 0.001}: gate 1, gate 2 and the same support."""
    _, G, H = issue_design(i)
    for rho in ec.DESIGN_RHO:
        lams = np.array(ec.DESIGN_FRACTIONS) * ec.lambda_max(H, rho).max()
        ref, _, conv, B, sweeps = ec.reference_path(G, H, lams, rho, tol=1e-12, snapshot_tol=1e-10)
        assert conv.all()
        n = ec.assert_gates(G[None], H[None], lams, rho, 1e-10, B[None], np.zeros((1, 4, 1), int), ref[None],
                            what=f"design {ec.DESIGNS[i]} rho={rho}")
        assert n == 4
        assert np.array_equal(B != 0, ref != 0)
        print(f"design {ec.DESIGNS[i]} rho={rho}: sweeps {sweeps[:, 0].tolist()}")


def test_the_cond_1e4_design_needs_many_sweeps():
    """What the status-1 test of the device rests on: at 0.01 lambda_max the reference needs at least 20 sweeps
    (max_sweeps = 2 cannot be enough), for every response used there."""
    _, G, H = issue_design(1, M=2)
    for rho in ec.DESIGN_RHO:
        lam = 0.01 * ec.lambda_max(H, rho).max()
        _, sweeps, conv = ec.reference_path(G, H, [lam], rho, tol=1e-8)
        assert conv.all() and sweeps.min() >= 20, sweeps


@pytest.mark.parametrize("K", ec.GRID_K)
def test_conditions_of_the_shape_grid(K):
    """Every case of the GPU shape grid, none left out: the reference converges at tol = 1e-12, needs at most
    max_sweeps / 2 sweeps from zero at the device's tolerance, mu > 0, and the support is decided at the device's
    tolerance (enet_cases.support_is_decided), so the count check of the GPU test applies to every problem."""
    for M in ec.GRID_M:
        for rho in ec.GRID_RHO:
            XTX, XTY, lams, ref = ec.grid_case(K, M, rho)
            assert np.all(np.isfinite(ref))
            for f in range(XTX.shape[0]):
                _, sweeps, conv = ec.reference_path(XTX[f], XTY[f], lams, rho, tol=ec.GPU_TOL)
                assert conv.all() and sweeps.max() <= ec.MAX_SWEEPS // 2, (K, M, rho, f, sweeps.max())
                assert np.all(lams < ec.lambda_max(XTY, rho).max()) and lams.min() >= 0.0099 * ec.lambda_max(XTY, rho).max()
                for l in range(lams.size):
                    for m in range(M):
                        assert ec.support_is_decided(XTX[f], XTY[f][:, m], ref[f, l, :, m], lams[l], rho, ec.GPU_TOL), \
                            (K, M, rho, f, l, m)


def test_conditions_of_the_route_cases():
    """The cases on each side of the kernel's route boundaries (enet_cases.ROUTE_CASES): the reference converges
    within max_sweeps / 2, and the dense ones have every coefficient nonzero at their smallest penalty."""
    for name in ec.ROUTE_CASES:
        XTX, XTY, lams, rho, ref, dense = ec.route_case(name)
        _, sweeps, conv = ec.reference_path(XTX[0], XTY[0], lams, rho, tol=ec.GPU_TOL)
        assert conv.all() and sweeps.max() <= ec.MAX_SWEEPS // 2, (name, sweeps.max())
        assert ec.strong_convexity(XTX[0], lams.min(), rho) > 0
        if dense:
            assert np.all(ref[0, -1] != 0), name
