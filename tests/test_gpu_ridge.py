"""GPU (-m gpu): the device ridge (cvm_ridge_fit through the C ABI) against NumPy float64 solves, against
ridge refitted from scratch on every training set, and against scikit-learn.

Tolerances.  A Cholesky solve is backward stable: the computed B solves a matrix within a small multiple
of K u ||A|| of A = XTX + lambda I, so ||A B - XTY||_F <= 1e-12 ||A||_F ||B||_F holds up to K = 4096
(u = 1.1e-16), and the forward error is at most cond(A) times that: 1e-10 where cond(A) <= 1e4.
Predictions from refits differ from ours by the conditioning of the same matrices times the rounding of
the fold stage's subtraction (XTX of all rows minus the validation rows): 1e-9 relative for the
well-conditioned designs used here.

The tests of the second half hold the kernel against oracle/ridge_oracle.py with the gate err <= 2 Y + 4 u
(float32: + 2^-24) of tests/ridge_cases.py, which is derived and not calibrated.  Where the kernel lands on the
MI355X (CVM_RIDGE_REPORT), largest err / Y per test and the case it came from:
  test_shape_grid            2.06  K = 31, M = 1, fold 2, lam = 1e-4 (2.3e-15 against 1.1e-15); median 1.18
  test_conditioning_ladder   1.57  K = 96, M = 3, cond 1e10, fold 3, lam = 0 (1.4e-7 against 8.8e-8); median 0.87
  test_every_problem_...     1.17  fold 13, penalty 7 (7.9e-16 against 6.8e-16), the same for every workspace
  test_limit_256_penalties   2.08  fold 1, penalty 94 (2.1e-15 against 9.9e-16)
  test_seeded_random_cases   1.92  draw 2, K = 32, M = 35, cond 81 (2.1e-15 against 1.1e-15); median 1.10
  float32 (grid, ladder, random): err at most 0.47, 0.49, 0.50 of 2^-24 -- the one rounding of the store
Before the panel update summed its products from zero the grid reached 3.07 (K = 256, M = 33,
lam = 10), the ladder 3.36, and test_shape_grid[127-1] missed its gate (3.85e-15 against 3.83e-15)."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ridge_cases as rc
from oracle import ridge_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rmod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import ridge as mod
    return mod


def spd_batch(rng, F, K, M, rows=None):
    n = rows or 2 * K + 3
    X = rng.standard_normal((F, n, K))
    XTX = np.einsum("fnk,fnj->fkj", X, X)
    XTX = 0.5 * (XTX + XTX.transpose(0, 2, 1))
    XTY = np.einsum("fnk,fnm->fkm", X, rng.standard_normal((F, n, M)))
    return XTX, XTY


def lam_grid(XTX, L):
    K = XTX.shape[-1]
    return np.logspace(-6, 2, L) * float(np.mean(np.trace(XTX, axis1=1, axis2=2))) / K


@pytest.mark.parametrize("K,M,F,L", [(1, 1, 3, 2), (7, 3, 5, 4), (33, 5, 7, 3), (127, 16, 4, 6), (512, 16, 10, 20),
                                     (1024, 32, 4, 3), (4096, 1, 2, 2)])
def test_against_numpy(rmod, K, M, F, L):
    rng = np.random.default_rng(K + M)
    XTX, XTY = spd_batch(rng, F, K, M)
    lam = lam_grid(XTX, L)
    fit = rmod.ridge_fit_batched(torch.from_numpy(XTX).cuda(), torch.from_numpy(XTY).cuda(), lam)
    B, info = fit.B.cpu().numpy(), fit.info.cpu().numpy()
    assert B.shape == (F, L, K, M) and info.shape == (F, L) and np.all(info == 0)
    I = np.eye(K)
    for f in range(F):
        for l in range(L):
            A = XTX[f] + lam[l] * I
            r = np.linalg.norm(A @ B[f, l] - XTY[f])
            assert r <= 1e-12 * np.linalg.norm(A) * np.linalg.norm(B[f, l]), (f, l, r)
            if K <= 1024:
                c = np.linalg.cond(A)
                if c <= 1e4:
                    ref = np.linalg.solve(A, XTY[f])
                    assert np.linalg.norm(B[f, l] - ref) <= 1e-10 * np.linalg.norm(ref), (f, l, c)


def test_float32(rmod):
    from cvmatrix_amd import CVMatrix
    rng = np.random.default_rng(3)
    N, K, M, P = 3000, 64, 3, 5
    X = rng.standard_normal((N, K)).astype(np.float32)
    Y = rng.standard_normal((N, M)).astype(np.float32)
    cvm = CVMatrix(True, True, False, False, dtype=np.float32)
    cvm.fit(X, Y)
    (XTX, XTY), _ = cvm.training_XTX_XTY_batched(cvm.prepare_folds([np.arange(N)[np.arange(N) % P == f] for f in range(P)]))
    lam = np.array([1.0, 10.0, 100.0])
    fit = rmod.ridge_fit_batched(XTX, XTY, lam)
    assert fit.B.dtype == torch.float32
    A64, Y64, B = XTX.double().cpu().numpy(), XTY.double().cpu().numpy(), fit.B.cpu().numpy()
    for f in range(P):
        for l, lv in enumerate(lam):
            ref = np.linalg.solve(A64[f] + lv * np.eye(K), Y64[f])
            assert np.linalg.norm(B[f, l] - ref) <= 1e-6 * np.linalg.norm(ref), (f, l)


def refit_predictions(X, Y, w, val, lam, flags, ddof=1):
    """Ridge refitted from scratch in NumPy on the training rows, standardised with the training set's
    weighted mean and std; predictions on the validation rows in the original units."""
    cx, cy, sx, sy = flags
    tr = np.setdiff1d(np.arange(X.shape[0]), val)
    wt = np.ones(tr.size) if w is None else w[tr]
    Xt, Yt = X[tr], Y[tr]
    mx = (wt @ Xt) / wt.sum() if (cx or sx) else np.zeros(X.shape[1])
    my = (wt @ Yt) / wt.sum() if (cx or cy or sy) else np.zeros(Y.shape[1])
    nz = np.count_nonzero(wt)
    dX = np.sqrt((wt @ (Xt - mx) ** 2) * nz / ((nz - ddof) * wt.sum())) if sx else np.ones(X.shape[1])
    dY = np.sqrt((wt @ (Yt - my) ** 2) * nz / ((nz - ddof) * wt.sum())) if sy else np.ones(Y.shape[1])
    Xs = (Xt - (mx if cx else 0)) / dX
    Ys = (Yt - (my if cy else 0)) / dY
    G, H = Xs.T @ (wt[:, None] * Xs), Xs.T @ (wt[:, None] * Ys)
    out = []
    for lv in lam:
        Bl = np.linalg.solve(G + lv * np.eye(X.shape[1]), H)
        out.append(((X[val] - (mx if cx else 0)) / dX) @ Bl * dY + (my if (cx or cy) else 0))   # centred X: mean of Y is the intercept
    return np.array(out)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("flags", [(True, True, True, True), (True, True, False, False), (False, False, False, False),
                                   (True, False, True, False)])
def test_end_to_end_against_refits(rmod, weighted, flags):
    """CVMatrix -> training_XTX_XTY_batched -> ridge_fit_batched -> pls_validation_sse against ridge refitted
    on every training set in NumPy.  Odd K through copy=False device tensors.  The designs have cond(XTX) of
    order 10, so the fold stage's rounding (a few u times ||XTX||) moves the coefficients by about 1e-14:
    predictions to 1e-9 relative, per-lambda SSE to 1e-9 relative."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import pls_validation_sse
    rng = np.random.default_rng(11)
    N, K, M, P = 900, 35, 3, 4
    X = rng.standard_normal((N, K)) + 0.5
    Y = X[:, :M] @ rng.standard_normal((M, M)) + 0.3 * rng.standard_normal((N, M)) + 1.0
    w = rng.random(N) + 0.1 if weighted else None
    labels = rng.integers(0, P, N)
    p = amd.Partitioner(labels)
    cvm = amd.CVMatrix(*flags, dtype=np.float64, copy=False)
    cvm.fit(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), None if w is None else torch.from_numpy(w).cuda())
    batch = cvm.prepare_folds(p)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    lam = np.array([1e-3, 1.0, 30.0, 1e3])
    fit = rmod.ridge_fit_batched(XTX, XTY, lam, check=True)
    sse, wsum = pls_validation_sse(cvm, batch, stats, fit.B)
    sse = sse.cpu().numpy()
    B = fit.B.cpu().numpy()
    muX, sdX, muY, sdY = (None if t is None else t.cpu().numpy() for t in stats)
    for f, key in enumerate(p.folds_dict):
        val = p.get_validation_indices(key)
        ref = refit_predictions(X, Y, w, val, lam, flags)
        Xs = X[val] - (muX[f] if muX is not None else 0)
        Xs = Xs / (sdX[f] if sdX is not None else 1)
        got = np.einsum("nk,lkm->lnm", Xs, B[f]) * (sdY[f] if sdY is not None else 1) + (muY[f] if muY is not None else 0)
        assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (f, np.abs(got - ref).max())
        wv = np.ones(val.size) if w is None else w[val]
        ref_sse = np.einsum("n,lnm->lm", wv, (ref - Y[val]) ** 2)
        np.testing.assert_allclose(sse[f], ref_sse, rtol=1e-9)


def test_against_sklearn(rmod):
    lm = pytest.importorskip("sklearn.linear_model")
    import cvmatrix_amd as amd
    rng = np.random.default_rng(5)
    N, K, M, P = 400, 12, 2, 5
    X = rng.standard_normal((N, K))
    Y = X @ rng.standard_normal((K, M)) + 0.5 * rng.standard_normal((N, M)) + 2.0
    labels = np.arange(N) % P
    lam = np.array([0.01, 1.0, 50.0])
    for w in (None, rng.random(N) + 0.2):
        cvm = amd.CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
        cvm.fit(X, Y, w)
        folds = [np.flatnonzero(labels == f) for f in range(P)]
        (XTX, XTY), (muX, _, muY, _) = cvm.training_XTX_XTY_batched(cvm.prepare_folds(folds))
        B = rmod.ridge_fit_batched(XTX, XTY, lam).B.cpu().numpy()
        muX, muY = muX.cpu().numpy(), muY.cpu().numpy()
        for f, val in enumerate(folds):
            tr = labels != f
            for l, lv in enumerate(lam):
                ref = lm.Ridge(alpha=lv, fit_intercept=True).fit(X[tr], Y[tr], None if w is None else w[tr]).predict(X[val])
                got = (X[val] - muX[f]) @ B[f, l] + muY[f]
                assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (f, l)
    # the example: cross-validated RMSE per lambda against the refits
    spec = importlib.util.spec_from_file_location("fast_cv_ridge", os.path.join(ROOT, "examples", "fast_cv_ridge.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    Y1 = Y[:, :1]
    got = ex.fast_cv_rmse(X, Y1, labels, lam)
    sse = np.zeros(lam.size)
    for f in range(P):
        val, tr = labels == f, labels != f
        for l, lv in enumerate(lam):
            pred = lm.Ridge(alpha=lv, fit_intercept=True).fit(X[tr], Y1[tr]).predict(X[val])
            sse[l] += ((pred.reshape(-1) - Y1[val].reshape(-1)) ** 2).sum()
    np.testing.assert_allclose(got[:, 0], np.sqrt(sse / N), rtol=1e-9)


def test_not_positive_definite(rmod):
    rng = np.random.default_rng(8)
    K, M = 40, 2
    XTX, XTY = spd_batch(rng, 3, K, M)
    Xr = rng.standard_normal((K // 2, K))                  # fold 1: fewer training rows than K
    XTX[1] = Xr.T @ Xr
    XTY[1] = Xr.T @ rng.standard_normal((K // 2, M))
    lam = np.array([0.0, 0.5, 5.0])
    t = lambda a: torch.from_numpy(a).cuda()          # noqa: E731
    fit = rmod.ridge_fit_batched(t(XTX), t(XTY), lam)
    B, info = fit.B.cpu().numpy(), fit.info.cpu().numpy()
    assert info[1, 0] > 0 and np.all(np.isnan(B[1, 0]))
    info[1, 0] = 0
    assert np.all(info == 0) and np.all(np.isfinite(B[:, 1:])) and np.all(np.isfinite(B[[0, 2], 0]))
    for f in range(3):
        for l in range(3):
            if (f, l) == (1, 0):
                continue
            ref = np.linalg.solve(XTX[f] + lam[l] * np.eye(K), XTY[f])
            assert np.linalg.norm(B[f, l] - ref) <= 1e-8 * np.linalg.norm(ref), (f, l)
    # lambda = 0 on a full-rank fold: least squares
    Xf = rng.standard_normal((200, K)); Yf = rng.standard_normal((200, M))
    B0 = rmod.ridge_fit_batched(t(Xf.T @ Xf), t(Xf.T @ Yf), [0.0]).B.cpu().numpy()[0, 0]
    ref = np.linalg.lstsq(Xf, Yf, rcond=None)[0]
    assert np.linalg.norm(B0 - ref) <= 1e-10 * np.linalg.norm(ref)
    with pytest.raises(np.linalg.LinAlgError, match="fold 1"):
        rmod.ridge_fit_batched(t(XTX), t(XTY), lam, check=True)


def test_bitwise_invariance(rmod):
    from cvmatrix_amd import _lib
    rng = np.random.default_rng(9)
    K, M, L = 200, 5, 20
    XTX, XTY = spd_batch(rng, 3, K, M)
    lam = lam_grid(XTX, L)
    A, Y = torch.from_numpy(XTX).cuda(), torch.from_numpy(XTY).cuda()
    ref = rmod.ridge_fit_batched(A, Y, lam)
    for _ in range(20):
        out = rmod.ridge_fit_batched(A, Y, lam)
        assert torch.equal(out.B, ref.B) and torch.equal(out.info, ref.info)
    # one fold alone == the same fold among 300 copies
    big = rmod.ridge_fit_batched(A[1:2].expand(300, K, K), Y[1:2].expand(300, K, M), lam[:2])
    alone = rmod.ridge_fit_batched(A[1:2], Y[1:2], lam[:2])
    for f in (0, 137, 299):
        assert torch.equal(big.B[f], alone.B[0])
    # one lambda alone == the same lambda inside the grid
    for l in (0, 7, 19):
        assert torch.equal(rmod.ridge_fit_batched(A, Y, lam[l:l + 1]).B[:, 0], ref.B[:, l])
    # through the C ABI with room for 1 or 3 problems only
    lib = _lib.load()
    one = lib.cvm_ridge_workspace_bytes(1, K, M, 1)
    lam_c = np.ascontiguousarray(lam)
    for n in (1, 3):
        ws = torch.empty(n * one, dtype=torch.uint8, device="cuda")
        B = torch.empty_like(ref.B)
        info = torch.empty_like(ref.info)
        rc = lib.cvm_ridge_fit(A.data_ptr(), Y.data_ptr(), 3, K, M, lam_c.ctypes.data, L, _lib.CVM_F64, B.data_ptr(),
                               info.data_ptr(), ws.data_ptr(), n * one, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(B, ref.B) and torch.equal(info, ref.info)


def test_argument_errors_at_the_c_abi(rmod):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    K, M, F = 8, 2, 2
    A = torch.eye(K, dtype=torch.float64, device="cuda").expand(F, K, K).contiguous()
    Y = torch.ones((F, K, M), dtype=torch.float64, device="cuda")
    B = torch.empty((F, 4, K, M), dtype=torch.float64, device="cuda")
    info = torch.empty((F, 4), dtype=torch.int32, device="cuda")
    one = lib.cvm_ridge_workspace_bytes(1, K, M, 1)
    ws = torch.empty(one, dtype=torch.uint8, device="cuda")
    good = np.array([0.0, 1.0, 2.0, 3.0])

    def call(lam=good, L=None, dtype=_lib.CVM_F64, Bp=None, nbytes=one, K_=K):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        return lib.cvm_ridge_fit(A.data_ptr(), Y.data_ptr(), F, K_, M, lam.ctypes.data if lam.size else None,
                                 lam.size if L is None else L, dtype, B.data_ptr() if Bp is None else Bp,
                                 info.data_ptr(), ws.data_ptr(), nbytes, None)

    for kwargs, code, text in (({"Bp": 0}, 1, b"null pointer"), ({"L": 0}, 1, b"1 <= L <= 256"),
                               ({"lam": np.ones(257)}, 1, b"1 <= L <= 256"), ({"lam": [1.0, -1.0]}, 1, b"finite and >= 0"),
                               ({"lam": [np.nan]}, 1, b"finite and >= 0"), ({"lam": [np.inf]}, 1, b"finite and >= 0"),
                               ({"dtype": 7}, 1, b"dtype"), ({"nbytes": one - 1}, 2, b"workspace too small"),
                               ({"K_": 4097}, 1, b"bad shape")):
        if kwargs.get("Bp") == 0:
            rc = lib.cvm_ridge_fit(A.data_ptr(), Y.data_ptr(), F, K, M, good.ctypes.data, 4, _lib.CVM_F64, None,
                                   info.data_ptr(), ws.data_ptr(), one, None)
        else:
            rc = call(**kwargs)
        assert rc == code, (kwargs, rc)
        assert text in lib.cvm_last_error(), (kwargs, lib.cvm_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.allclose(B[:, 1], Y / 2.0)


# ---------------------------------------------------------------------------------------------------------
# The kernel against an extended-precision reference (oracle/ridge_oracle.py; fixtures and the gate in
# tests/ridge_cases.py, whose own conditions tests/test_ridge_oracle.py checks on the CPU).

needs_longdouble = pytest.mark.skipif(not ro.LONGDOUBLE_OK, reason=ro.LONGDOUBLE_REASON)
GRID_LAMBDAS = np.array([0.0, 1e-4, 10.0])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit_np(rmod, XTX, XTY, lam):
    fit = rmod.ridge_fit_batched(dev(XTX), dev(XTY), lam)
    return fit.B.cpu().numpy(), fit.info.cpu().numpy()


def cabi_fit(XTX, XTY, lam, slots=None, ws_fill=None, B_fill=None, info_fill=None):
    """cvm_ridge_fit through the C ABI on device tensors, with a workspace of `slots` problems (None: what
    cvm_ridge_workspace_bytes asks for) that holds `ws_fill` in every byte beforehand."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = XTY.shape
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    L = lam.size
    one = lib.cvm_ridge_workspace_bytes(1, K, M, 1)
    nbytes = lib.cvm_ridge_workspace_bytes(F, K, M, L) if slots is None else slots * one
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    B = torch.empty((F, L, K, M), dtype=XTX.dtype, device="cuda")
    info = torch.empty((F, L), dtype=torch.int32, device="cuda")
    if B_fill is not None:
        B.fill_(B_fill)
    if info_fill is not None:
        info.fill_(info_fill)
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    rc_ = lib.cvm_ridge_fit(XTX.data_ptr(), XTY.data_ptr(), F, K, M, lam.ctypes.data, L, code, B.data_ptr(),
                            info.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc_ == 0, lib.cvm_last_error()
    torch.cuda.synchronize()
    return B, info


def same_bits(a, b):
    """Bitwise equality, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_batch(rmod, XTX, XTY, lam, what):
    B, info = fit_np(rmod, XTX, XTY, lam)
    F, K, M = XTY.shape
    assert B.shape == (F, len(lam), K, M) and B.dtype == XTX.dtype and np.all(info == 0), (what, info)
    ref, Y = rc.references(XTX, XTY, lam)
    worst = rc.assert_gate(B, ref, Y, what, float32=XTX.dtype == np.float32)
    print(f"{what}: largest err / Y = {worst:.2f}")
    return B


@needs_longdouble
@pytest.mark.parametrize("K,M", rc.GRID)
def test_shape_grid(rmod, K, M):
    """(a) Every tile count of the back substitution, short last panels and bottom blocks, K + M just
    below, on and above a multiple of 32: three distinct folds x [0, small, large] against the reference."""
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(1000 * K + M), 3, K, M, 1e2)
    check_batch(rmod, XTX, XTY, GRID_LAMBDAS, f"grid K={K} M={M}")


@pytest.mark.parametrize("K,M,F,L", [(4096, 64, 1, 2), (1024, 64, 3, 2)])
def test_largest_slots(rmod, K, M, F, L):
    """(a) K = 4096 with M = 64 is the largest slot the header allows: the residual gate of test_against_numpy."""
    rng = np.random.default_rng(K + M)
    XTX, XTY = spd_batch(rng, F, K, M, rows=K + 64)
    lam = lam_grid(XTX, L)
    B, info = fit_np(rmod, XTX, XTY, lam)
    assert np.all(info == 0)
    for f in range(F):
        for l in range(L):
            A = XTX[f] + lam[l] * np.eye(K)
            r = np.linalg.norm(A @ B[f, l] - XTY[f])
            assert r <= 1e-12 * np.linalg.norm(A) * np.linalg.norm(B[f, l]), (f, l, r)


@needs_longdouble
@pytest.mark.parametrize("cond", rc.LADDER_COND)
@pytest.mark.parametrize("K,M", rc.LADDER_KM)
def test_conditioning_ladder(rmod, K, M, cond):
    """(b) Forward error where it is cond(A) u and not u: a kernel that is merely residual-consistent
    (or loses digits in the back substitution) fails here and nowhere else."""
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(int(100 * K + M + np.log10(cond))), 6, K, M, cond)
    check_batch(rmod, XTX, XTY, rc.ladder_lambdas(cond), f"ladder K={K} M={M} cond={cond:.0e}")


@needs_longdouble
@pytest.mark.parametrize("K,M", rc.GRID_F32)
def test_float32_shape_grid(rmod, K, M):
    """(c) float32 in and out: one float32 rounding on top of the float64 gate, as the header promises."""
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(1000 * K + M + 1), 3, K, M, 1e2, np.float32)
    check_batch(rmod, XTX, XTY, GRID_LAMBDAS, f"grid32 K={K} M={M}")


@needs_longdouble
@pytest.mark.parametrize("cond", rc.LADDER_COND_F32)
@pytest.mark.parametrize("K,M", rc.LADDER_KM)
def test_float32_conditioning_ladder(rmod, K, M, cond):
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(int(100 * K + M + np.log10(cond)) + 1), 6, K, M, cond, np.float32)
    check_batch(rmod, XTX, XTY, rc.ladder_lambdas(cond), f"ladder32 K={K} M={M} cond={cond:.0e}")


INFO_LAMBDAS = np.array([0.0, 1e-3])


def check_one_bad_fold(rmod, XTX, XTY, want, lam=INFO_LAMBDAS, bad_fold=1):
    """Fold `bad_fold` fails at pivot `want` at every penalty with B all NaN; every other problem has the
    bits it has when its fold is run alone."""
    B, info = fit_np(rmod, XTX, XTY, lam)
    assert np.all(info[bad_fold] == want), (want, info)
    assert np.all(np.isnan(B[bad_fold]))
    for f in range(XTX.shape[0]):
        if f != bad_fold:
            Ba, ia = fit_np(rmod, XTX[f:f + 1], XTY[f:f + 1], lam)
            assert np.all(ia == 0) and np.all(info[f] == 0) and np.all(np.isfinite(Ba))
            assert same_bits(B[f], Ba[0]), (want, f)
    return B


@pytest.mark.parametrize("K", rc.INFO_K)
def test_info_is_the_pivot_lapack_names(rmod, K):
    """(d) A well-conditioned matrix made indefinite at pivot j (tests/test_ridge_oracle.py: the oracle and
    dpotrf name j, with a pivot below -1e-3 ||A||_2): info == j exactly, in the first panel, on a panel's
    first and last column, in the short last panel."""
    for j in rc.info_pivots(K):
        XTX, XTY = rc.indefinite_fixture(K, j)
        for lv in INFO_LAMBDAS:
            assert ro.cholesky_info(XTX[1] + lv * np.eye(K))[0] == j
        check_one_bad_fold(rmod, XTX, XTY, j)


@pytest.mark.parametrize("K", rc.INFO_K)
def test_info_on_non_finite_input(rmod, K):
    """(d) NaN and +Inf on the diagonal at j: info == j.  NaN at a symmetric off-diagonal pair (i, j), i > j:
    the first pivot it reaches is i.  The oracle is asked every time."""
    rng = np.random.default_rng(K)
    good, XTY = rc.spd_spectrum(rng, 4, K, 3, 1e2)
    for j in rc.info_pivots(K):
        for v in (np.nan, np.inf):
            XTX = good.copy()
            XTX[1, j - 1, j - 1] = v
            assert ro.cholesky_info(XTX[1])[0] == j
            check_one_bad_fold(rmod, XTX, XTY, j)
    # what a fold of status 1 hands over: NaN throughout
    XTX, XTYn = good.copy(), XTY.copy()
    XTX[1], XTYn[1] = np.nan, np.nan
    check_one_bad_fold(rmod, XTX, XTYn, 1)
    for i, j in ((K, 1), (K, K - 1), (34, 2), (40, 33), (64, 31), (65, 64), (K - 1, 32)):
        if j < i <= K:
            XTX = good.copy()
            XTX[1, i - 1, j - 1] = XTX[1, j - 1, i - 1] = np.nan
            assert ro.cholesky_info(XTX[1])[0] == i
            check_one_bad_fold(rmod, XTX, XTY, i)


@pytest.mark.parametrize("K,M", [(33, 5), (70, 17), (100, 40)])
def test_nan_in_xty_only(rmod, K, M):
    """(d) NaN in XTY alone: the factorisation succeeds (info == 0), the columns of B that had a NaN in
    their right-hand side are NaN, every other column and every other problem has the bits it has
    without the NaN (include/cvmhip.h says so)."""
    rng = np.random.default_rng(K + M)
    XTX, XTY = rc.spd_spectrum(rng, 3, K, M, 1e2)
    lam = INFO_LAMBDAS
    clean, info0 = fit_np(rmod, XTX, XTY, lam)
    assert np.all(info0 == 0)
    dirty = XTY.copy()
    cols = sorted({0, M // 2, M - 1})
    rows = [K - 1, K // 2, 0]
    for c, r in zip(cols, rows):
        dirty[1, r, c] = np.nan
    B, info = fit_np(rmod, XTX, dirty, lam)
    assert np.all(info == 0)
    keep = [m for m in range(M) if m not in cols]
    assert np.all(np.isnan(B[1][:, :, cols])) and np.all(np.isfinite(B[1][:, :, keep]))
    assert same_bits(B[1][:, :, keep], clean[1][:, :, keep])
    assert same_bits(B[[0, 2]], clean[[0, 2]])


def test_float32_failure(rmod):
    """(c) One failing problem in float32: info as in float64, B all NaN in float32."""
    for K, j in ((70, 33), (33, 33), (100, 64)):
        XTX, XTY = rc.indefinite_fixture(K, j, np.float32)
        info_o, piv = ro.cholesky_info(XTX[1].astype(np.float64))
        assert info_o == j and rc.info_is_unambiguous(XTX[1], info_o, piv)
        B = check_one_bad_fold(rmod, XTX, XTY, j)
        assert B.dtype == np.float32


@pytest.mark.parametrize("slots", [1, 2])
def test_a_workgroup_survives_a_failed_problem(rmod, slots):
    """(e) Eight problems through one or two workgroups, the 1st, 4th and last of them failing: the healthy
    ones as in a full-workspace run, the failed ones NaN with their own pivot."""
    K, M = 70, 5
    rng = np.random.default_rng(21)
    XTX, XTY = rc.spd_spectrum(rng, 8, K, M, 1e2)
    want = np.zeros((8, 1), dtype=np.int32)
    for f, j in ((0, 40), (3, 3), (7, 70)):
        rc.make_indefinite(XTX[f], j)
        want[f] = j
        assert ro.cholesky_info(XTX[f])[0] == j
    A, Yd = dev(XTX), dev(XTY)
    full_B, full_info = cabi_fit(A, Yd, [0.0])
    B, info = cabi_fit(A, Yd, [0.0], slots=slots)
    assert np.array_equal(info.cpu().numpy(), want) and np.array_equal(full_info.cpu().numpy(), want)
    B, full_B = B.cpu().numpy(), full_B.cpu().numpy()
    for f in range(8):
        if want[f]:
            assert np.all(np.isnan(B[f])) and np.all(np.isnan(full_B[f]))
        else:
            assert np.all(np.isfinite(B[f]))
            r = np.linalg.norm(XTX[f] @ B[f, 0] - XTY[f])
            assert r <= 1e-12 * np.linalg.norm(XTX[f]) * np.linalg.norm(B[f, 0])
    assert same_bits(B, full_B)


@needs_longdouble
def test_every_problem_is_solved_once_whatever_the_workspace(rmod):
    """(f) 40 distinct folds x 15 penalties through workspaces of 1 to 512 problems: the map from workgroup
    to problem and from problem to (fold, penalty) leaves no problem out, solves none with another's fold
    or penalty, and does not change a bit."""
    K, M, F, L = 5, 2, 40, 15
    rng = np.random.default_rng(31)
    XTX, XTY = rc.spd_spectrum(rng, F, K, M, 1e2)
    lam = np.logspace(-3, 1, L)
    ref, Y = rc.references(XTX, XTY, lam)
    A, Yd = dev(XTX), dev(XTY)
    sentinel = -12345.678
    first = None
    for slots in (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512):
        B, info = cabi_fit(A, Yd, lam, slots=slots, B_fill=sentinel, info_fill=-7)
        B, info = B.cpu().numpy(), info.cpu().numpy()
        assert not np.any(B == sentinel) and np.all(info == 0), slots
        rc.assert_gate(B, ref, Y, f"dealing G={slots}")
        if first is None:
            first = B
        assert same_bits(B, first), slots
    # the distinct folds and penalties are told apart by the gate: the nearest wrong answer is far outside it
    assert ro.rel_err(ref[1, 0], ref[0, 0]) > 1e-3 and ro.rel_err(ref[0, 1], ref[0, 0]) > 1e-6 > rc.gate_bound(Y.max())


@pytest.mark.parametrize("K,M", [(33, 3), (70, 17), (100, 64), (257, 33)])
def test_workspace_content_does_not_matter(rmod, K, M):
    """(g) The slot is read past row R in MFMA operands whose outputs are not stored: NaN, huge finite values
    and zeros there give the same bits, with and without a failing problem in the batch."""
    rng = np.random.default_rng(K * M)
    XTX, XTY = rc.spd_spectrum(rng, 5, K, M, 1e2)
    lam = INFO_LAMBDAS
    for bad in (False, True):
        if bad:
            rc.make_indefinite(XTX[2], min(K, 40))
        A, Yd = dev(XTX), dev(XTY)
        outs = [cabi_fit(A, Yd, lam, slots=s, ws_fill=fill) for fill in (0xFF, 0x7F, 0x00) for s in (None, 2)]
        B0, i0 = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
        assert np.all(i0[[0, 1, 3, 4]] == 0) and np.all(np.isfinite(B0[[0, 1, 3, 4]]))
        assert np.all(i0[2] == (min(K, 40) if bad else 0)) and np.all(np.isnan(B0[2])) == bad
        for B, info in outs[1:]:
            assert same_bits(B.cpu().numpy(), B0) and same_bits(info.cpu().numpy(), i0)


@needs_longdouble
def test_limit_256_penalties(rmod):
    """(h) L = 256: the 2 KB kernel argument.  Every column against the reference; three of them bitwise
    against the single-penalty call."""
    K, M, F = 40, 3, 2
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(256), F, K, M, 1e2)
    lam = np.logspace(-6, 3, 256)
    B = check_batch(rmod, XTX, XTY, lam, "L=256")
    for l in (0, 131, 255):
        Bl, _ = fit_np(rmod, XTX, XTY, lam[l:l + 1])
        assert same_bits(Bl[:, 0], B[:, l]), l


def test_limit_huge_penalty(rmod):
    """(h) lam = 1e300: A is lam I to 1e-300, so B = XTY / lam.  In relative Frobenius norm (the measure of
    every gate in this file) within two roundings, 2 u.  Element-wise a Cholesky cannot promise that:
    B = (y / d) / d with d = fl(sqrt(lam)) carries two division roundings and twice the rounding of the
    root, d^2 = lam (1 - 0.82 u) at 1e300: at most 2.82 u for an element, so every element is held to 3 u.
    Measured: 0.98 u in norm, 2.11 u for the worst element."""
    K, M = 40, 3
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(300), 3, K, M, 1e2)
    B, info = fit_np(rmod, XTX, XTY, [1e300, 1.0])
    assert np.all(info == 0)
    exact = XTY.astype(np.longdouble) / np.longdouble(1e300)
    d = B[:, 0].astype(np.longdouble) - exact
    err = float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(exact * exact)))
    print(f"lam=1e300: normwise {err / rc.U:.2f} u, largest element {float(np.max(np.abs(d / exact))) / rc.U:.2f} u")
    assert err <= 2 * rc.U
    assert float(np.max(np.abs(d / exact))) <= 3 * rc.U


def test_limit_shapes_and_views(rmod):
    """(h) F = 0; a single (K, K) with (K,); non-contiguous inputs against their contiguous copies."""
    K, M = 33, 4
    XTX, XTY = rc.spd_spectrum(np.random.default_rng(5), 3, K, M, 1e2)
    A, Yd = dev(XTX), dev(XTY)
    lam = [0.5, 2.0]
    empty = rmod.ridge_fit_batched(A[:0], Yd[:0], lam, check=True)
    assert empty.B.shape == (0, 2, K, M) and empty.info.shape == (0, 2) and empty.B.dtype == torch.float64
    ref = rmod.ridge_fit_batched(A, Yd, lam)
    one = rmod.ridge_fit_batched(A[1], Yd[1, :, 2], lam)
    assert one.B.shape == (1, 2, K, 1) and torch.equal(one.info, torch.zeros_like(one.info))
    col = rmod.ridge_fit_batched(A[1:2], Yd[1:2, :, 2:3].contiguous(), lam)
    assert torch.equal(one.B, col.B)
    want = np.linalg.solve(XTX[1] + 0.5 * np.eye(K), XTY[1, :, 2])
    assert np.linalg.norm(one.B[0, 0, :, 0].cpu().numpy() - want) <= 1e-12 * np.linalg.norm(want)
    # a transposed view (XTX symmetric in exact bits here: the fixture is symmetrised) and a view of XTY
    At = A.transpose(1, 2)
    assert not At.is_contiguous() and torch.equal(At, A)
    Yt = Yd.transpose(1, 2).contiguous().transpose(1, 2)
    assert not Yt.is_contiguous()
    out = rmod.ridge_fit_batched(At, Yt, lam)
    assert torch.equal(out.B, ref.B) and torch.equal(out.info, ref.info)
    # an expanded fold (stride 0)
    Ae, Ye = A[2:3].expand(4, K, K), Yd[2:3].expand(4, K, M)
    assert not Ae.is_contiguous()
    out = rmod.ridge_fit_batched(Ae, Ye, lam)
    for f in range(4):
        assert torch.equal(out.B[f], ref.B[2])


def test_end_to_end_wide_y(rmod):
    """(i) test_end_to_end_against_refits once more with three tiles of responses, K = 70 and 64 penalties."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import pls_validation_sse
    rng = np.random.default_rng(13)
    N, K, M, P = 1200, 70, 40, 4
    flags = (True, True, True, True)
    X = rng.standard_normal((N, K)) + 0.5
    Y = X[:, :M] @ rng.standard_normal((M, M)) + 0.3 * rng.standard_normal((N, M)) + 1.0
    w = rng.random(N) + 0.1
    labels = rng.integers(0, P, N)
    p = amd.Partitioner(labels)
    cvm = amd.CVMatrix(*flags, dtype=np.float64, copy=False)
    cvm.fit(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda())
    batch = cvm.prepare_folds(p)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    lam = np.logspace(-3, 3, 64)
    fit = rmod.ridge_fit_batched(XTX, XTY, lam, check=True)
    sse, wsum = pls_validation_sse(cvm, batch, stats, fit.B)
    sse = sse.cpu().numpy()
    B = fit.B.cpu().numpy()
    muX, sdX, muY, sdY = (t.cpu().numpy() for t in stats)
    for f, key in enumerate(p.folds_dict):
        val = p.get_validation_indices(key)
        ref = refit_predictions(X, Y, w, val, lam, flags)
        got = np.einsum("nk,lkm->lnm", (X[val] - muX[f]) / sdX[f], B[f]) * sdY[f] + muY[f]
        assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (f, np.abs(got - ref).max())
        ref_sse = np.einsum("n,lnm->lm", w[val], (ref - Y[val]) ** 2)
        np.testing.assert_allclose(sse[f], ref_sse, rtol=1e-9)


@needs_longdouble
def test_seeded_random_cases(rmod):
    """(j) 150 seeded draws of shape, dtype, conditioning and penalties, one in ten with an indefinite fold.
    info against the oracle wherever its call is unambiguous (test_ridge_oracle.py: at least nine draws in
    ten); the accuracy gate for every penalty of every draw: the reference has to exist for all the healthy
    folds (the generator keeps to conditioning at which it converges), and the gated pairs are counted."""
    worst, compared, gated, pairs = (0.0, None), 0, 0, 0
    for d in rc.random_draws():
        XTX, XTY, lam = d["XTX"], d["XTY"], d["lam"]
        what = f"draw {d['i']} K={d['K']} M={d['M']} F={d['F']} L={d['L']} {np.dtype(d['dtype']).name} cond={d['cond']:.1e}"
        B, info = fit_np(rmod, XTX, XTY, lam)
        want, sure = rc.oracle_info(XTX, lam)
        assert np.array_equal(info[sure], want[sure]), (what, info, want)
        compared += bool(sure.all())
        assert np.all(np.isnan(B[info != 0])) and np.all(np.isfinite(B[info == 0])), what
        healthy = [f for f in range(d["F"]) if f != d["bad_fold"]]
        if d["bad_fold"] is not None:
            assert np.all(info[d["bad_fold"]] > 0), what
        for l in range(d["L"]):
            pairs += 1
            try:
                ref, Y = rc.references(XTX[healthy], XTY[healthy], lam[l:l + 1])
            except np.linalg.LinAlgError:
                continue
            assert np.all(info[healthy, l] == 0), what
            r = rc.assert_gate(B[healthy, l:l + 1], ref, Y, f"{what} l={l}", float32=d["dtype"] == np.float32)
            if d["dtype"] == np.float64:          # (float32: the error is the rounding of the store, not Y)
                worst = max(worst, (r, what))
            gated += 1
    assert compared * 10 >= 9 * rc.RANDOM_DRAWS
    assert gated == pairs, (gated, pairs)
    print(f"random: {gated} of {pairs} (draw, penalty) pairs gated; float64: largest err / Y = {worst[0]:.2f} at {worst[1]}")
