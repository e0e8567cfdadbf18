"""CPU: the reference of tests/pcr_cases.py against another LAPACK driver and against scikit-learn, and the
host half of the device PCR -- workspace sizing through the C ABI (host arithmetic, no device query), the
checks of A and rank_tol and the refusal of host tensors before any device is touched."""

import numpy as np
import pytest
import torch

import pcr_cases as pc
from cvmatrix_amd import _lib
from cvmatrix_amd import pcr


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def designs(K):
    rng = np.random.default_rng(K)
    out = [("wishart", pc.wishart(rng, K), range(0)), ("low rank", pc.low_rank(rng, K, max(1, K // 3)), range(0))]
    if K >= 2:
        out.append(("graded 2", pc.graded(rng, K, 2), range(min(K, 8))))
    if K >= 5:
        out.append(("clustered", pc.clustered(rng, K), (0, 3)))
    return out


@pytest.mark.parametrize("K", [1, 2, 3, 7, 33, 64, 129])
def test_reference_agrees_with_the_evr_driver(K):
    """numpy.linalg.eigh (LAPACK evd) against scipy.linalg.eigh(driver="evr") through the same rank rule and
    formula: the backward gates on every design, the coefficients where the gate applies."""
    sl = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(100 + K)
    for name, G, parity in designs(K):
        A = min(K, 8) if name != "clustered" else 4
        H = pc.responses(rng, K, 3)
        B, lam, V, n_fit = pc.pcr_reference(G, H, A)
        lam2, V2 = sl.eigh(G, driver="evr")
        B2, lam2, V2, n_fit2 = pc.reference_from_eig(lam2[::-1], V2[:, ::-1], H, A, pc.default_rank_tol(K))
        what = f"{name} K={K}"
        assert n_fit == n_fit2, what
        for vv, ll, other in ((V, lam, lam2), (V2, lam2, lam)):
            pc.assert_backward(G, vv[:, :n_fit], ll[:n_fit], other[:n_fit], what)
        pc.assert_coefficients(B2, B, [a for a in parity if a < A], what)
        pc.assert_consistency(B, V, lam, H, n_fit, what)


def test_reference_is_sklearn_pcr():
    dec = pytest.importorskip("sklearn.decomposition")
    lm = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(4)
    N, K, M, A = 200, 9, 2, 5
    X = rng.standard_normal((N, 4)) @ rng.standard_normal((4, K)) + 0.3 * rng.standard_normal((N, K)) + 1.0
    Y = X[:, :M] + 0.2 * rng.standard_normal((N, M)) - 2.0
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    B, lam, V, n_fit = pc.pcr_reference(Xc.T @ Xc, Xc.T @ Yc, A)
    assert n_fit == A
    for a in range(A):
        p = dec.PCA(n_components=a + 1, svd_solver="full").fit(X)
        reg = lm.LinearRegression().fit(p.transform(X), Y)
        ref = p.components_.T @ reg.coef_.T
        assert np.linalg.norm(B[a] - ref) <= 1e-9 * np.linalg.norm(ref), a
        pred = reg.predict(p.transform(X[:7]))
        assert np.abs((X[:7] - X.mean(0)) @ B[a] + Y.mean(0) - pred).max() <= 1e-9 * np.abs(pred).max()


def test_workspace_bytes_is_host_arithmetic(lib):
    for K, M in ((1, 0), (1, 1), (1, 64), (7, 3), (33, 64), (64, 64), (257, 33), (512, 16), (512, 0), (511, 64)):
        one = lib.cvm_pcr_workspace_bytes(1, K, M, 1)
        ld = (max(K, M) + 3) // 4 * 4
        assert one == (2 * K * ld * 8 + 255) // 256 * 256 > 0
        for F, A in ((1, 1), (3, K), (10, min(K, 20)), (511, 1), (512, 1), (513, 1), (100000, K)):
            assert lib.cvm_pcr_workspace_bytes(F, K, M, A) == min(F, 512) * one, (K, M, F, A)
        assert lib.cvm_pcr_workspace_bytes(0, K, M, 1) == one          # (room for one fold at the least)


def test_workspace_bytes_is_monotone(lib):
    ws = lib.cvm_pcr_workspace_bytes
    for K in range(1, 512):
        assert ws(10, K + 1, 16, 1) >= ws(10, K, 16, 1)
    for M in range(0, 64):
        assert ws(10, 40, M + 1, 8) >= ws(10, 40, M, 8)
    for F in range(1, 700, 7):
        assert ws(F + 1, 256, 4, 8) >= ws(F, 256, 4, 8)
    # out of range: 0 (the caller sees a workspace that cannot hold a fold)
    assert ws(1, 0, 1, 1) == 0 and ws(1, 513, 1, 1) == 0 and ws(1, 8, 1, 9) == 0 and ws(1, 8, 65, 1) == 0
    assert ws(1, 8, 1, 0) == 0 and ws(-1, 8, 1, 1) == 0 and ws(1, 8, -1, 1) == 0


def test_host_tensors_are_refused_before_the_device():
    with pytest.raises(TypeError):
        pcr.pcr_fit_batched(torch.eye(3, dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64), 2)
    with pytest.raises(TypeError):
        pcr.pcr_fit_batched(np.eye(3), np.ones((3, 1)), 2)
    with pytest.raises(TypeError):
        pcr.pcr_fit_batched(torch.eye(3, dtype=torch.float64), None, 2)


@pytest.mark.parametrize("A", [0, -1, 9, 2.0, "2", None, True])
def test_bad_component_count_is_refused(A):
    with pytest.raises(ValueError):
        pcr.check_components(A, 8)


@pytest.mark.parametrize("tol", [float("nan"), 1.0, 2.5, float("inf")])
def test_bad_rank_tol_is_refused(tol):
    with pytest.raises(ValueError):
        pcr.check_rank_tol(tol)


def test_good_arguments_are_accepted():
    assert pcr.check_components(np.int64(8), 8) == 8 and pcr.check_components(1, 8) == 1
    assert pcr.check_rank_tol(None) == 0.0 and pcr.check_rank_tol(-3.0) == 0.0 and pcr.check_rank_tol(0) == 0.0
    assert pcr.check_rank_tol(1e-8) == 1e-8
    assert pcr.default_rank_tol(33) == pc.default_rank_tol(33) == 32 * 33 * 2.0 ** -52
