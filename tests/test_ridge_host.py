"""CPU: the host half of the device ridge -- workspace sizing through the C ABI (host arithmetic, no
device query), the penalty-grid checks and the refusal of host tensors before any device is touched."""

import numpy as np
import pytest
import torch

from cvmatrix_amd import _lib
from cvmatrix_amd import ridge


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_workspace_bytes_is_host_arithmetic(lib):
    for K, M in ((1, 1), (7, 3), (512, 16), (1024, 32), (4096, 1), (100, 64), (257, 33), (4096, 64)):
        one = lib.cvm_ridge_workspace_bytes(1, K, M, 1)
        ld = (K + M + 31) // 32 * 32
        assert one == (K * ld * 8 + 255) // 256 * 256 > 0
        for F, L in ((1, 1), (3, 2), (10, 20), (100, 10), (64, 10), (1, 256), (600, 1)):
            assert lib.cvm_ridge_workspace_bytes(F, K, M, L) == min(F * L, 512) * one, (K, M, F, L)


def test_workspace_bytes_is_monotone(lib):
    ws = lib.cvm_ridge_workspace_bytes
    for K in (1, 31, 32, 33, 100, 1000, 4095):
        assert ws(10, K + 1, 16, 20) >= ws(10, K, 16, 20)
    for M in range(1, 64):
        assert ws(10, 512, M + 1, 20) >= ws(10, 512, M, 20)
    for P in range(1, 700, 7):
        assert ws(P + 1, 256, 4, 1) >= ws(P, 256, 4, 1)
    # out of range: 0 (the caller sees a workspace that cannot hold a problem)
    assert ws(1, 0, 1, 1) == 0 and ws(1, 4097, 1, 1) == 0 and ws(1, 8, 65, 1) == 0 and ws(1, 8, 1, 257) == 0


@pytest.mark.parametrize("bad", [[-1.0], [0.5, np.nan], [np.inf], [], np.ones(257), np.ones((2, 2)), [[1.0]]])
def test_penalty_grid_is_refused(bad):
    with pytest.raises(ValueError):
        ridge.check_lambdas(bad)


def test_penalty_grid_is_accepted():
    lam = ridge.check_lambdas([0, 1e-6, 3, 1e300])
    assert lam.dtype == np.float64 and lam.flags.c_contiguous and lam.shape == (4,)
    assert ridge.check_lambdas(np.ones(256)).size == 256
    assert ridge.check_lambdas(2.0 * np.arange(5)[::2]).tolist() == [0.0, 4.0, 8.0]


def test_host_tensors_are_refused_before_the_device():
    with pytest.raises(TypeError):
        ridge.ridge_fit_batched(torch.eye(3, dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64), [1.0])
    with pytest.raises(TypeError):
        ridge.ridge_fit_batched(np.eye(3), np.ones((3, 1)), [1.0])
