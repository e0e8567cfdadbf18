"""GPU (-m gpu): the device ridge (cvm_ridge_fit through the C ABI) against NumPy float64 solves, against
ridge refitted from scratch on every training set, and against scikit-learn.

Tolerances.  A Cholesky solve is backward stable: the computed B solves a matrix within a small multiple
of K u ||A|| of A = XTX + lambda I, so ||A B - XTY||_F <= 1e-12 ||A||_F ||B||_F holds up to K = 4096
(u = 1.1e-16), and the forward error is at most cond(A) times that: 1e-10 where cond(A) <= 1e4.
Predictions from refits differ from ours by the conditioning of the same matrices times the rounding of
the fold stage's subtraction (XTX of all rows minus the validation rows): 1e-9 relative for the
well-conditioned designs used here."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

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
