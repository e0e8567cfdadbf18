"""CPU: the host half of the device orthogonal matching pursuit -- the argument rules of cvmatrix_amd/omp.py
before any device is touched, the workspace sizing and the argument errors of the C ABI -- and the conditions the
GPU tests (tests/test_gpu_omp.py) rest on: the NumPy reference of tests/omp_cases.py against scikit-learn's
orthogonal_mp_gram, gate 2 on the reference itself, and, for every case of the GPU shape grid, that every
selection is decided beyond the rounding of the scores."""

import ctypes

import numpy as np
import pytest
import torch

import omp_cases as oc
from cvmatrix_amd import _lib
from cvmatrix_amd import omp


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


A3 = torch.eye(3, dtype=torch.float64)
Y3 = torch.ones((3, 1), dtype=torch.float64)


@pytest.mark.parametrize("bad", [0, 65, 2.5, -1, True, "3", None, np.float64(2.0)])
def test_the_number_of_variables_is_refused(bad):
    with pytest.raises(ValueError):
        omp.check_selected(bad, 4096)
    with pytest.raises(ValueError):
        omp.omp_fit_batched(A3, Y3, bad)          # (before the tensors are looked at: they are host tensors)


def test_the_number_of_variables_against_K():
    for K in (1, 3, 64, 100):
        with pytest.raises(ValueError):
            omp.check_selected(K + 1, K)
        assert omp.check_selected(min(K, 64), K) == min(K, 64)
    assert omp.check_selected(np.int64(7), 9) == 7 and type(omp.check_selected(np.int32(7), 9)) is int
    assert omp.MAX_SELECTED == 64 and omp.MAX_K == 4096 and omp.MAX_RESPONSES == 64 and omp.WORKSPACE_LIMIT > 0


@pytest.mark.parametrize("bad", [np.nan, 1.0, 2.0, np.inf])
def test_rank_tol_is_refused(bad):
    with pytest.raises(ValueError):
        omp.check_rank_tol(bad)
    with pytest.raises(ValueError):
        omp.omp_fit_batched(A3, Y3, 1, rank_tol=bad)


def test_rank_tol_is_accepted():
    assert omp.check_rank_tol(None) == 0.0 and omp.check_rank_tol(0) == 0.0 and omp.check_rank_tol(-3.0) == 0.0
    assert omp.check_rank_tol(1e-9) == 1e-9 and omp.check_rank_tol(0.999) == 0.999
    assert omp.default_rank_tol(20) == 32 * 20 * 2.0 ** -52 == oc.default_rank_tol(20)


def test_host_tensors_are_refused_before_the_device():
    with pytest.raises(TypeError):
        omp.omp_fit_batched(A3, Y3, 2)
    with pytest.raises(TypeError):
        omp.omp_fit_batched(np.eye(3), np.ones((3, 1)), 2, normalize=True)
    assert issubclass(omp.OMPRankWarning, RuntimeWarning) and omp.OMPFit._fields == ("B", "support", "n_fit")


def test_workspace_bytes_is_host_arithmetic(lib):
    ws = lib.cvm_omp_workspace_bytes
    for K in (1, 31, 32, 33, 512, 4096):
        A = min(K, 20)
        one = ws(1, K, 1, 1)
        assert one == (8 * K + 255) // 256 * 256
        for F, M, a in ((1, 1, 1), (3, 17, A), (10, 16, A), (100, 16, A), (16, 64, 1), (17, 64, min(K, 64))):
            assert ws(F, K, M, a) == min(F * M, 1024) * one, (K, F, M, a)
    assert ws(0, 8, 1, 1) == ws(1, 8, 1, 1)
    assert ws(1, 0, 1, 1) == 0 and ws(1, 4097, 1, 1) == 0 and ws(1, 8, 65, 1) == 0 and ws(1, 8, 0, 1) == 0
    assert ws(1, 8, 1, 0) == 0 and ws(1, 8, 1, 9) == 0 and ws(1, 100, 1, 65) == 0 and ws(-1, 8, 1, 1) == 0


def test_argument_errors_are_decided_before_the_device(lib):
    """K = 0 and 4097, M = 0 and 65, A = 0, K + 1 and 65, normalize 2, rank_tol NaN and 1, a dtype that is none, a
    null pointer: CVM_EINVAL from arguments alone (the pointers are never followed); n_folds == 0 launches nothing;
    less than one slot is CVM_EWORKSPACE."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(K=8, M=2, A=3, normalize=0, rank_tol=0.0, dtype=_lib.CVM_F64, F=0, XTX=p, ws_bytes=256):
        return lib.cvm_omp_fit(XTX, p, F, K, M, A, normalize, rank_tol, dtype, p, p, p, p, ws_bytes, None)

    assert call() == _lib.CVM_OK                                   # no fold: nothing is launched
    for kw, text in (({"K": 0}, b"K"), ({"K": 4097}, b"K"), ({"M": 0}, b"M"), ({"M": 65}, b"M"), ({"A": 0}, b"A"),
                     ({"A": 9}, b"A"), ({"K": 100, "A": 65}, b"A"), ({"normalize": 2}, b"normalize"),
                     ({"rank_tol": float("nan")}, b"rank_tol"), ({"rank_tol": 1.0}, b"rank_tol"),
                     ({"dtype": 7}, b"dtype"), ({"XTX": None}, b"null"), ({"F": -1}, b"shape")):
        assert call(**kw) == _lib.CVM_EINVAL, kw
        assert text in lib.cvm_last_error(), (kw, lib.cvm_last_error())
    assert call(K=33, ws_bytes=511) == _lib.CVM_EWORKSPACE
    assert call(K=33, ws_bytes=512) == _lib.CVM_OK


@pytest.mark.parametrize("K,M,A", [(2, 3, 2), (63, 3, 5), (64, 1, 64), (65, 17, 64), (130, 3, 64), (257, 1, 64)])
def test_reference_against_sklearn(K, M, A):
    """orthogonal_mp_gram(G, h, n_nonzero_coefs=A, return_path=True) on the plain designs of the grid: the same
    supports in the same order, the coefficients of every step to 1e-10 relative in norm (cond(G_SS) <= 4 there:
    loose by five orders)."""
    lm = pytest.importorskip("sklearn.linear_model")
    XTX, XTY, (support, n_fit, B, _) = oc.grid_case(K, M, A, False)
    for f in range(XTX.shape[0]):
        for m in range(M):
            path = lm.orthogonal_mp_gram(XTX[f], XTY[f][:, m], n_nonzero_coefs=A, return_path=True)
            path = path.reshape(K, -1)                                       # (K, A)
            assert n_fit[f, m] == A == path.shape[1]
            for a in range(A):
                got = np.flatnonzero(path[:, a])
                assert np.array_equal(np.sort(support[f, :a + 1, m]), got), (f, m, a)
                assert np.linalg.norm(path[:, a] - B[f, a, :, m]) <= 1e-10 * np.linalg.norm(path[:, a]), (f, m, a)
            # the order of selection: the variable that enters at step a
            order = [int(np.setdiff1d(np.flatnonzero(path[:, a]), np.flatnonzero(path[:, a - 1]) if a else [])[0])
                     for a in range(A)]
            assert order == support[f, :, m].tolist(), (f, m)


@pytest.mark.parametrize("K", oc.GRID_K)
def test_conditions_of_the_shape_grid(K):
    """Every case of the GPU shape grid, none left out: every path selects all A variables, every selection is
    decided (margin >= 100 e, omp_cases.assert_decided) with cond(G_SS) <= 100 (of the equilibrated G_SS on the
    rescaled designs of normalize=True), and the reference's own coefficients pass gate 2."""
    for M in oc.GRID_M:
        for A in oc.grid_A(K):
            for normalize in (False, True):
                what = f"K={K} M={M} A={A} normalize={normalize}"
                XTX, XTY, ref = oc.grid_case(K, M, A, normalize)
                assert np.all(ref[1] == A), what
                worst, rel, cond, cond_eq = oc.assert_decided(XTX, XTY, A, normalize, ref, normalize, what)
                frac = oc.assert_second_gate(XTX, XTY, ref[0], ref[1], ref[2], what=what)
                print(f"{what}: margin at least {worst:.3g} e = {rel:.3g} of the largest score; cond(G_SS) at most "
                      f"{cond:.3g} ({cond_eq:.3g} equilibrated); the reference at {frac:.3f} of gate 2")


def test_the_two_criteria_select_differently():
    """On the rescaled design, |alpha| and |alpha| / sqrt(G_kk) pick different variables (else normalize=True
    would be tested by nothing), and on a design with equal column norms they agree."""
    K, M, A = 65, 3, 5
    XTX, XTY, (support, _, _, _) = oc.grid_case(K, M, A, True)
    plain = oc.reference_batch(XTX, XTY, A, False)[0]
    assert not np.array_equal(plain, support)
    r = 1.0 / np.sqrt(np.diagonal(XTX, axis1=1, axis2=2))
    unit = XTX * r[:, :, None] * r[:, None, :]
    assert np.array_equal(oc.reference_batch(unit, XTY * r[:, :, None], A, False)[0],
                          oc.reference_batch(unit, XTY * r[:, :, None], A, True)[0])


def test_the_edge_designs():
    """What the GPU edge tests expect of the rule itself: the exact tie takes index 2 and never index 5, the
    rank-r design stops at r with the padding of the last model, h = 0 selects nothing, a zero column is never
    selected under normalize=True."""
    G, H = oc.tie_case()
    support, n, coef, _ = oc.reference(G[0], H[0][:, 0], 8)
    assert support[0] == 2 and 5 not in support and n == 7 and support[7] == -1
    XTX, XTY = oc.low_rank_case(r=4)
    for f in range(2):
        for m in range(2):
            support, n, coef, _ = oc.reference(XTX[f], XTY[f][:, m], 6)
            assert n == 4 and np.all(support[:4] < 4) and np.all(support[4:] == -1)
            assert np.array_equal(coef[4], coef[3]) and np.array_equal(coef[5], coef[3])
    support, n, coef, _ = oc.reference(XTX[0], np.zeros(8), 3)
    assert n == 0 and np.all(support == -1) and not coef.any()
    Gz = XTX[0][:4, :4].copy()
    Gz[2, :] = Gz[:, 2] = 0.0
    hz = XTY[0][:4, 0].copy()
    hz[2] = 0.0
    support, n, _, _ = oc.reference(Gz, hz, 4, normalize=True)
    assert n == 3 and 2 not in support
