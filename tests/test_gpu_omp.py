"""GPU (-m gpu): the device orthogonal matching pursuit (cvm_omp_fit, cvmatrix_amd/omp.py) against the two gates of
tests/omp_cases.py -- support and n_fit equal to the NumPy reference's exactly, the backward error of a Cholesky
solve for the coefficients of every step -- and its contract: the lane and piece boundaries, the exact tie, the
early stop and its padding, non-finite inputs, bit-reproducibility whatever the batch and the workspace,
``check=True``, and the pipeline end to end.

The conditions gate 1 rests on (every selection of every grid case decided by at least 100 times the rounding of
the scores) are asserted on the CPU in tests/test_omp_host.py.  Each test prints the largest fraction of gate 2 it
attained; on the MI355X the shape grid lands at most at 0.36 of the bound in float64 (the NumPy reference itself:
0.36) and at 0.98 in float32, where the bound is the rounding of the store itself."""

import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import omp_cases as oc

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def omod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import omp as mod
    return mod


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the fixtures are read-only)


def fit_np(omod, XTX, XTY, A, dtype=np.float64, **kw):
    fit = omod.omp_fit_batched(dev(XTX, dtype), dev(XTY, dtype), A, **kw)
    assert fit.B.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    assert fit.support.dtype == fit.n_fit.dtype == torch.int32
    return fit.B.cpu().numpy(), fit.support.cpu().numpy(), fit.n_fit.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_case(omod, XTX, XTY, A, normalize, ref, dtype, what):
    """Both gates for every path of a case; returns (B, the attained fraction of gate 2)."""
    F, K, M = XTY.shape
    B, support, n_fit = fit_np(omod, XTX, XTY, A, dtype, normalize=normalize)
    assert B.shape == (F, A, K, M) and support.shape == (F, A, M) and n_fit.shape == (F, M)
    assert np.array_equal(n_fit, ref[1]), (what, n_fit, ref[1])
    assert np.array_equal(support, ref[0]), (what, np.argwhere(support != ref[0])[:5])
    frac = oc.assert_second_gate(XTX, XTY, support, n_fit, B, float32=dtype == np.float32, what=what)
    print(f"{what}: {frac:.3f} of gate 2")
    return B, frac


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("normalize", (False, True), ids=("plain", "normalized"))
@pytest.mark.parametrize("steps", (0, 1, 2), ids=("one", "five", "all"))
@pytest.mark.parametrize("M", oc.GRID_M)
@pytest.mark.parametrize("K", oc.GRID_K)
def test_shape_grid(omod, K, M, steps, normalize, dtype):
    """K on both sides of the 64 lanes and of the 256-coordinate piece, M on both sides of a fold's share of an
    XCD, A = 1, min(K, 5) and min(K, 64) (K = 64: every column is selected; K >= 64: every lane holds a variable),
    three folds with different matrices; normalize=True on columns whose norms spread over 1 .. 30."""
    A = (1, min(K, 5), min(K, 64))[steps]
    XTX, XTY, ref = oc.grid_case(K, M, A, normalize)
    B, _ = check_case(omod, XTX, XTY, A, normalize, ref, dtype,
                      f"grid K={K} M={M} A={A} normalize={normalize} {np.dtype(dtype).name}")
    if K == 64 and A == 64:
        assert np.all(B[:, -1] != 0)


def test_the_two_criteria_select_differently_on_the_device(omod):
    K, M, A = 65, 3, 5
    XTX, XTY, ref = oc.grid_case(K, M, A, True)
    _, plain, _ = fit_np(omod, XTX, XTY, A, normalize=False)
    _, scaled, _ = fit_np(omod, XTX, XTY, A, normalize=True)
    assert np.array_equal(scaled, ref[0]) and not np.array_equal(plain, scaled)
    assert np.array_equal(plain, oc.reference_batch(XTX, XTY, A, False)[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_exact_tie_takes_the_lowest_index(omod, dtype):
    """Columns 2 and 5 identical to the bit: index 2 is selected (first: the strongest coefficient is there), index
    5 never -- once 2 is in, its pivot is zero -- so the path of 8 steps ends after 7."""
    G, H = oc.tie_case()
    G, H = G.astype(np.float32).astype(np.float64), H.astype(np.float32).astype(np.float64)
    ref = oc.reference(G[0], H[0][:, 0], 8)
    B, support, n_fit = fit_np(omod, G, H, 8, dtype)
    assert support[0, 0, 0] == 2 and 5 not in support[0, :, 0] and n_fit[0, 0] == 7 and support[0, 7, 0] == -1
    assert np.array_equal(support[0, :, 0], ref[0])
    assert np.all(B[0, :, 5, 0] == 0) and same_bits(B[0, 7], B[0, 6])
    oc.assert_second_gate(G, H, support, n_fit, B, float32=dtype == np.float32, what="tie")
    # fewer steps: the same path, cut short
    B3, support3, _ = fit_np(omod, G, H, 3, dtype)
    assert support3[0, 0, 0] == 2 and same_bits(B3[0], B[0, :3])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_early_stop_and_padding(omod, dtype):
    """Rank r = 4 in 8 columns (the second half copies of the first), A = 6: n_fit == 4, support -1 from step 4
    on, B[f, a >= 4] the bits of B[f, 3].  h = 0: nothing is selected, B is all zero.  normalize=True never selects a
    zero column."""
    r, A = 4, 6
    XTX, XTY = oc.low_rank_case(r)
    XTX, XTY = XTX.astype(np.float32).astype(np.float64), XTY.astype(np.float32).astype(np.float64)
    for normalize in (False, True):
        B, support, n_fit = fit_np(omod, XTX, XTY, A, dtype, normalize=normalize)
        assert np.all(n_fit == r) and np.all(support[:, r:] == -1) and np.all(support[:, :r] >= 0)
        assert np.all(support[:, :r] < r)                                  # (of two equal columns the lower index)
        for a in range(r, A):
            assert same_bits(B[:, a], B[:, r - 1])
        ref = oc.reference_batch(XTX, XTY, A, normalize)
        assert np.array_equal(support, ref[0]) and np.array_equal(n_fit, ref[1])
        oc.assert_second_gate(XTX, XTY, support, n_fit, B, float32=dtype == np.float32, what="rank 4")
    # one response all zero beside one that is not
    XTY0 = XTY.copy()
    XTY0[:, :, 1] = 0.0
    B, support, n_fit = fit_np(omod, XTX, XTY0, A, dtype)
    assert np.all(n_fit[:, 1] == 0) and np.all(support[:, :, 1] == -1) and not B[:, :, :, 1].any()
    assert np.all(n_fit[:, 0] == r) and np.all(np.signbit(B[:, :, :, 1]) == 0)
    # a zero column
    G = XTX[:, :r, :r].copy()
    G[:, 2, :] = G[:, :, 2] = 0.0
    Hz = XTY[:, :r].copy()
    Hz[:, 2] = 0.0
    B, support, n_fit = fit_np(omod, G, Hz, r, dtype, normalize=True)
    assert np.all(n_fit == r - 1) and not np.any(support == 2) and not B[:, :, 2].any()
    with pytest.warns(omod.OMPRankWarning, match="path"):
        omod.omp_fit_batched(dev(XTX, dtype), dev(XTY, dtype), A, check=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", omod.OMPRankWarning)
        omod.omp_fit_batched(dev(XTX, dtype), dev(XTY, dtype), r, check=True)          # all r selected: no warning


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_not_finite(omod, dtype):
    """A NaN on the diagonal of one fold's XTX: that fold all NaN with n_fit -1 and support -1, the other folds
    the bits of a run without it.  A NaN in one column of XTY: that response only.  An off-diagonal NaN or infinity
    in a row the path reads: n_fit -1, never a finite wrong number."""
    K, M, A = 65, 3, 5
    XTX, XTY, ref = oc.grid_case(K, M, A, False)
    clean = fit_np(omod, XTX, XTY, A, dtype)
    bad_G, bad_H = XTX.copy(), XTY.copy()
    bad_G[2, 40, 40] = np.nan
    bad_H[1, 7, 1] = np.nan
    B, support, n_fit = fit_np(omod, bad_G, bad_H, A, dtype)
    want = np.zeros((3, M), bool)
    want[2] = True
    want[1, 1] = True
    assert np.array_equal(n_fit == -1, want) and np.array_equal(n_fit[~want], clean[2][~want])
    assert np.array_equal(np.isnan(B).all(axis=(1, 2)), want) and np.array_equal(np.isnan(B).any(axis=(1, 2)), want)
    assert np.all(support.transpose(0, 2, 1)[want] == -1)
    for f in range(3):
        for m in range(M):
            if not want[f, m]:
                assert same_bits(B[f, :, :, m], clean[0][f, :, :, m]) and same_bits(support[f, :, m], clean[1][f, :, m])
    with pytest.raises(np.linalg.LinAlgError, match="fold 1, response 1"):
        omod.omp_fit_batched(dev(bad_G, dtype), dev(bad_H, dtype), A, check=True)
    # an infinity in h; a NaN or an infinity off the diagonal, in the row of the first variable that response 0 of
    # fold 0 selects: that path reads it at its second step
    for value in (np.nan, np.inf):
        bad_G, bad_H = XTX.copy(), XTY.copy()
        j = int(ref[0][0, 0, 0])
        k = (j + 9) % K
        bad_G[0, j, k] = bad_G[0, k, j] = value
        bad_H[1, 3, 2] = np.inf
        B, support, n_fit = fit_np(omod, bad_G, bad_H, A, dtype)
        assert n_fit[0, 0] == -1 and n_fit[1, 2] == -1 and np.all(n_fit[2] == A)
        for f in range(3):
            for m in range(M):
                # a path either read the entry and says so, or has the bits of the clean run
                if n_fit[f, m] == -1:
                    assert (f == 0 or (f, m) == (1, 2)) and np.all(np.isnan(B[f, :, :, m])) and np.all(support[f, :, m] == -1)
                else:
                    assert same_bits(B[f, :, :, m], clean[0][f, :, :, m]) and same_bits(support[f, :, m], clean[1][f, :, m])


def cabi_fit(XTX, XTY, A, normalize=0, rank_tol=0.0, paths=None):
    """cvm_omp_fit through the C ABI with a workspace of `paths` slots (None: what the library asks for)."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = XTY.shape
    one = lib.cvm_omp_workspace_bytes(1, K, 1, A)
    nbytes = lib.cvm_omp_workspace_bytes(F, K, M, A) if paths is None else paths * one
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    B = torch.full((F, A, K, M), -7.0, dtype=XTX.dtype, device="cuda")
    support = torch.full((F, A, M), -7, dtype=torch.int32, device="cuda")
    n_fit = torch.full((F, M), -7, dtype=torch.int32, device="cuda")
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_omp_fit(XTX.data_ptr(), XTY.data_ptr(), F, K, M, A, normalize, rank_tol, code, B.data_ptr(),
                         support.data_ptr(), n_fit.data_ptr(), ws.data_ptr(), nbytes,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cvm_last_error()
    torch.cuda.synchronize()
    return B, support, n_fit


def test_reproducible_whatever_the_batch_and_the_workspace(omod):
    """Two runs are bit-equal; a fold alone has the bits it has in the batch; F M = 9 paths through workspaces of
    one slot, of four and of all nine give the same bits (ws_bytes handed to the C entry); the explicit default
    rank_tol is the implicit one."""
    K, M, A = 130, 3, 64
    XTX, XTY, _ = oc.grid_case(K, M, A, True)
    G, H = dev(XTX), dev(XTY)
    first = omod.omp_fit_batched(G, H, A, normalize=True)
    again = omod.omp_fit_batched(G, H, A, normalize=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert torch.all(first.n_fit == A)
    alone = omod.omp_fit_batched(G[1], H[1], A, normalize=True)
    assert torch.equal(alone.B[0], first.B[1]) and torch.equal(alone.support[0], first.support[1])
    one = omod.omp_fit_batched(G[2], H[2, :, 1], A, normalize=True)
    assert one.B.shape == (1, A, K, 1) and torch.equal(one.B[0, :, :, 0], first.B[2, :, :, 1])
    for paths in (1, 4, None):
        B, support, n_fit = cabi_fit(G, H, A, 1, 0.0, paths)
        assert torch.equal(B, first.B) and torch.equal(support, first.support) and torch.equal(n_fit, first.n_fit), paths
    B, _, _ = cabi_fit(G, H, A, 1, omod.default_rank_tol(A))
    assert torch.equal(B, first.B)
    empty = omod.omp_fit_batched(G[:0], H[:0], A, check=True)
    assert empty.B.shape == (0, A, K, M) and empty.support.shape == (0, A, M) and empty.n_fit.shape == (0, M)


def test_more_paths_than_workgroups(omod):
    """F = 70 folds x M = 17 responses = 1190 paths, more than the 1024 in flight: the bits of the same folds run
    in two halves, and both gates on a sample."""
    F, M, K, A = 70, 17, 8, 3
    XTX, XTY = oc.fold_matrices(60, K, M, A, F=F, seed=3)
    G, H = dev(XTX), dev(XTY)
    whole = omod.omp_fit_batched(G, H, A)
    lo, hi = omod.omp_fit_batched(G[:35], H[:35], A), omod.omp_fit_batched(G[35:], H[35:], A)
    for w, a, b in zip(whole, lo, hi):
        assert torch.equal(w, torch.cat([a, b]))
    for f in (0, 34, 35, 69):
        ref = oc.reference_batch(XTX[f:f + 1], XTY[f:f + 1], A)
        oc.assert_decided(XTX[f:f + 1], XTY[f:f + 1], A, False, ref, False, f"fold {f}")
        assert np.array_equal(whole.support[f:f + 1].cpu().numpy(), ref[0])
        oc.assert_second_gate(XTX[f:f + 1], XTY[f:f + 1], ref[0], ref[1], whole.B[f:f + 1].cpu().numpy(), what=f"fold {f}")


def test_python_limits_on_device_tensors(omod):
    G = torch.eye(5, dtype=torch.float64, device="cuda")
    for bad in (6, 0):
        with pytest.raises(ValueError):
            omod.omp_fit_batched(G, G[:, :2], bad)
    with pytest.raises(ValueError):
        omod.omp_fit_batched(G, torch.ones((5, 65), dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(ValueError):
        omod.omp_fit_batched(G, G[:, :0], 2)
    with pytest.raises(ValueError):
        omod.omp_fit_batched(torch.eye(4097, dtype=torch.float32, device="cuda"),
                             torch.ones((4097, 1), dtype=torch.float32, device="cuda"), 2)
    fit = omod.omp_fit_batched(G, torch.arange(5.0, dtype=torch.float64, device="cuda"), 5, check=False)
    assert fit.support[0, :, 0].tolist() == [4, 3, 2, 1, -1] and int(fit.n_fit) == 4     # (h_0 = 0: nothing left)


def test_example_against_sklearn(omod):
    """examples/fast_cv_omp.py at N = 300, K = 24, M = 2, five folds, A = 6, centred: the RMSE per number of
    variables against scikit-learn's OrthogonalMatchingPursuit refitted on every training set.  Both solve the same
    least-squares problems on supports of cond <= 100: cond K u is 1e-13, the tolerance 1e-8 relative."""
    pytest.importorskip("sklearn.linear_model")
    spec = importlib.util.spec_from_file_location("fast_cv_omp", os.path.join(ROOT, "examples", "fast_cv_omp.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, Y, labels, A = oc.sklearn_cv_problem()
    rmse, support = ex.fast_cv_rmse(X, Y, labels, A)
    assert rmse.shape == (A, Y.shape[1]) and support.shape == (5, A, Y.shape[1])
    ref = ex.sklearn_cv_rmse(X, Y, labels, A)
    np.testing.assert_allclose(rmse, ref, rtol=1e-8)
    assert np.all(np.diff(rmse[:5], axis=0) < 0)             # (five and six true variables: the RMSE falls)


def test_hand_on_to_cv_predict(omod):
    """cv_predict(cvm, folds, stats, fit.B) takes the stack: the reference and the gate of tests/predict_cases.py."""
    import predict_cases as pc
    import cvmatrix_amd as amd
    from cvmatrix_amd.predict import cv_predict
    pc.require_longdouble()
    X, Y, labels, A = oc.sklearn_cv_problem()
    folds = [np.flatnonzero(labels == f) for f in range(5)]
    cvm = amd.CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    fit = omod.omp_fit_batched(XTX, XTY, A, check=True)
    out = cv_predict(cvm, batch, stats, fit.B, order="folds").cpu().numpy()
    ref, gate = pc.cv_reference(cvm.X.cpu().numpy(), folds, fit.B.cpu().numpy(),
                                tuple(None if s is None else s.cpu().numpy() for s in stats))
    pc.assert_gate(out, ref, gate, "cv_predict on the OMP stack")
