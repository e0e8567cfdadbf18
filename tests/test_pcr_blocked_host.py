"""CPU: the NumPy model of the blocked eigensolver (tests/pcr_blocked_cases.py) against the reference of
tests/pcr_cases.py inside the project's gates on the designs the GPU tests use, and the host half of
cvm_pcr_blocked_fit -- workspace sizing through the C ABI (host arithmetic, no device query) and the argument rules
of pcr_fit_batched(solver=..., max_sweeps=...), all before any device is touched."""

import numpy as np
import pytest
import torch

import pcr_blocked_cases as bc
import pcr_cases as pc
from cvmatrix_amd import _lib
from cvmatrix_amd import pcr

b = pcr.BLOCK


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_constants():
    assert pcr.BLOCK == 32 and pcr.MAX_K_BLOCKED == 4096 and pcr.MAX_K == 512


@pytest.mark.parametrize("K", bc.host_K(b))
def test_model_within_the_gates(K):
    """The method itself on Wishart, graded (ratio 2), clustered and rank-3 designs: the backward gates on the
    components that exist, the coefficients where the split is well separated, the consistency gate."""
    rng = np.random.default_rng(2000 + K)
    cases = (("wishart", pc.wishart(rng, K), 8, ()), ("graded 2", pc.graded(rng, K, 2), 8, range(8)),
             ("clustered", pc.clustered(rng, K), 4, (0, 3)), ("rank 3", pc.low_rank(rng, K, 3), 8, ()))
    for name, G, A, parity in cases:
        what = f"{name} K={K}"
        H = pc.responses(rng, K, 3)
        Bref, lref, Vref, nref = pc.pcr_reference(G, H, A)
        lam, V, sweeps = bc.block_jacobi_model(G, b)
        assert 1 <= sweeps <= bc.MAX_SWEEPS, (what, sweeps)
        assert np.all(np.diff(lam) <= 0), what
        B, la, Va, n_fit = pc.reference_from_eig(lam, V, H, A, pc.default_rank_tol(K))
        assert n_fit == nref == (3 if name == "rank 3" else A), (what, n_fit, nref)
        Vs = pc.align_signs(Va[:, :n_fit], Vref[:, :n_fit])
        figs = pc.assert_backward(G, Vs, la[:n_fit], lref[:n_fit], what)
        pc.assert_coefficients(B, Bref, parity, what)
        pc.assert_consistency(B, Va, la, H, n_fit, what)
        # every eigenvalue, not the leading ones alone
        assert np.max(np.abs(lam - np.linalg.eigvalsh(G)[::-1])) <= pc.backward_bound(K) * np.linalg.norm(G), what
        print(f"model {what}: {sweeps} sweeps, residual {figs[0]:.1e}, orthogonality {figs[1]:.1e}, eigenvalues "
              f"{figs[2]:.1e} against {pc.backward_bound(K):.1e}")


def test_model_trivial_matrices():
    K = 2 * b + 1
    lam, V, sweeps = bc.block_jacobi_model(np.eye(K), b)
    assert sweeps == 1 and np.array_equal(lam, np.ones(K)) and np.array_equal(V, np.eye(K))
    lam, V, sweeps = bc.block_jacobi_model(np.zeros((K, K)), b)
    assert sweeps == 1 and not np.any(lam)
    G = pc.wishart(np.random.default_rng(5), 129)
    assert bc.block_jacobi_model(G, b, max_sweeps=1)[2] == -1


def slot_bytes(K, M):
    """A slot as include/cvmhip.h describes it: S and V padded to Kp, Kp / 64 matrices Q, the coefficient sum,
    the signs and the threshold in float64; the ordering, the flag words and the status array in int32."""
    m = bc.blocks_even(K, b)
    Kp, h = m * b, m // 2
    doubles = 2 * Kp * Kp + h * (2 * b) ** 2 + K * M + Kp + 2
    ints = Kp + h + 8 + 512
    return (doubles * 8 + ints * 4 + 255) // 256 * 256


def test_workspace_bytes_is_host_arithmetic(lib):
    ws = lib.cvm_pcr_blocked_workspace_bytes
    for K, M in ((1, 0), (1, 64), (b, 3), (b + 1, 1), (2 * b + 1, 64), (513, 2), (1024, 32), (4095, 1), (4096, 64)):
        one = ws(1, K, M, 1)
        assert one == slot_bytes(K, M) > 0 and one % 256 == 0, (K, M)
        for F, A in ((1, 1), (3, K), (511, 1), (512, 1), (513, 1), (100000, K)):
            assert ws(F, K, M, A) == min(F, 512) * one, (K, M, F, A)
        assert ws(0, K, M, 1) == one
    assert 2 * 4096 * 4096 * 8 < ws(1, 4096, 1, 16) < 272 * 10 ** 6      # "about 270 MB"


def test_workspace_bytes_is_monotone_and_refuses_bad_shapes(lib):
    ws = lib.cvm_pcr_blocked_workspace_bytes
    for F in range(1, 700, 7):
        assert ws(F + 1, 257, 4, 8) >= ws(F, 257, 4, 8)
    assert ws(512, 257, 4, 8) == ws(513, 257, 4, 8) == ws(10 ** 6, 257, 4, 8)
    for K in range(1, 700, 3):
        assert ws(10, K + 1, 16, 1) >= ws(10, K, 16, 1)
    assert ws(1, 0, 1, 1) == 0 and ws(1, 4097, 1, 1) == 0 and ws(1, 8, 1, 9) == 0 and ws(1, 8, 65, 1) == 0
    assert ws(1, 8, 1, 0) == 0 and ws(-1, 8, 1, 1) == 0 and ws(1, 8, -1, 1) == 0
    assert ws(1, 513, 1, 1) > 0 and ws(1, 4096, 1, 1) > 0
    # the scalar entry keeps its limit
    assert lib.cvm_pcr_workspace_bytes(1, 513, 1, 1) == 0


HOST_G, HOST_H = torch.eye(3, dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64)


@pytest.mark.parametrize("solver", ["block", "", None, "BLOCKED", 1])
def test_bad_solver_is_refused(solver):
    with pytest.raises(ValueError):
        pcr.pcr_fit_batched(HOST_G, HOST_H, 2, solver=solver)


@pytest.mark.parametrize("sweeps", [0, -1, 61, 2.0, "3", True])
def test_bad_max_sweeps_is_refused(sweeps):
    with pytest.raises(ValueError):
        pcr.pcr_fit_batched(HOST_G, HOST_H, 2, solver="blocked", max_sweeps=sweeps)


def test_max_sweeps_goes_with_the_blocked_solver():
    for sweeps in (1, 30, 60):
        with pytest.raises(ValueError):
            pcr.pcr_fit_batched(HOST_G, HOST_H, 2, max_sweeps=sweeps)
        with pytest.raises(ValueError):
            pcr.pcr_fit_batched(HOST_G, HOST_H, 2, solver="scalar", max_sweeps=sweeps)


def test_host_tensors_are_refused_before_the_device():
    for kw in ({"solver": "blocked"}, {"solver": "blocked", "max_sweeps": 7}, {"solver": "scalar"}):
        with pytest.raises(TypeError):
            pcr.pcr_fit_batched(HOST_G, HOST_H, 2, **kw)
        with pytest.raises(TypeError):
            pcr.pcr_fit_batched(np.eye(3), np.ones((3, 1)), 2, **kw)
        with pytest.raises(TypeError):
            pcr.pcr_fit_batched(HOST_G, None, 2, **kw)


def test_the_scalar_solver_keeps_its_limit():
    big = torch.zeros((1, 513, 513))
    with pytest.raises(ValueError, match="512"):
        pcr.pcr_fit_batched(big, None, 1)
    with pytest.raises(ValueError, match="512"):
        pcr.pcr_fit_batched(big, None, 1, solver="scalar")
    with pytest.raises(ValueError, match="4096"):
        pcr.pcr_fit_batched(torch.zeros((1, 1, 4097)).expand(1, 4097, 4097), None, 1, solver="blocked")
    with pytest.raises(TypeError):                    # K = 513 is in range for the blocked solver: next rule
        pcr.pcr_fit_batched(big, None, 1, solver="blocked")
