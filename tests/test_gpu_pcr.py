"""GPU (-m gpu): the device PCA / PCR (cvm_pcr_fit through pcr_fit_batched and the C ABI) against the
reference, the designs and the gates of tests/pcr_cases.py, whose own conditions tests/test_pcr_host.py
checks on the CPU.  The gates are derived there, not calibrated; every test prints where the kernel lands
(run with -s).  On the MI355X, the largest figure over the folds of a test (residual, orthogonality,
eigenvalues, each against 60 K u; sweeps):
  test_shape_grid      K = 32   1.1e-15  4.8e-15  4.1e-16  against 2.1e-13   8 sweeps
                       K = 129  1.7e-15  2.6e-14  4.3e-16  against 8.6e-13   10 sweeps
  test_upper_limit     K = 512  3.9e-15  1.3e-13  7.4e-16  against 3.4e-12   12 sweeps, 1.9 s
  test_graded_spectra  K = 64   2.2e-15  2.1e-14  6.7e-16  against 4.3e-13   17..18 sweeps (the most seen)
                       K = 257  4.7e-15  8.2e-14  2.4e-15  against 1.7e-12   13 sweeps
  test_clusters        K = 129  1.5e-15  1.1e-14  4.2e-16  against 8.6e-13   5..6 sweeps
Coefficients against the reference (gate 1e-10): graded at most 1.5e-13 (K = 129), clustered a = 0, 3 at most
1.0e-14; float32 3.5e-8 against 1e-10 + 2^-24 = 6.0e-8.  Consistency: below 0.005 of its bound in every test.
With a plain float64 sum for the scores v^T XTY in the kernel and in the rebuild, test_shape_grid[65-1] and
[257-1] missed the gate (3.7 and 1.3 times the bound at a = 0, where the score nearly cancels); the kernel's sum
is now compensated and the rebuild takes the scores rounded once (pcr_cases.exact_dot)."""

import ctypes

import numpy as np
import pytest
import torch

import pcr_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pmod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import pcr as mod
    return mod


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit_np(pmod, G, H, A, **kw):
    """pcr_fit_batched on NumPy stacks; everything back as NumPy."""
    fit = pmod.pcr_fit_batched(dev(G), None if H is None else dev(H), A, return_components=True, **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in fit)


def same_bits(a, b):
    """Bitwise equality, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_fit(x, y):
    return all(same_bits(p, q) for p, q in zip(x, y))


def stack(rng, make, F, K, M):
    G = np.stack([make(rng, K) for _ in range(F)])
    H = np.stack([pc.responses(rng, K, M) for _ in range(F)])
    return G, H


def check_fold(G, H, A, out, f, what, parity=(), n_fit=None):
    """The backward gates, the sign convention and the consistency gate on fold f of `out`; coefficient
    parity on the components in `parity`.  Returns the figures."""
    B, lam, V, nf, sweeps = (t[f] for t in out)
    K = G.shape[-1]
    want = A if n_fit is None else n_fit
    assert nf == want, (what, nf)
    assert 1 <= sweeps <= pc.MAX_SWEEPS, (what, sweeps)
    assert np.all(np.diff(lam) <= 0), (what, lam)
    Bref, lref, Vref, nref = pc.pcr_reference(G[f], H[f], A)
    assert nref == want, what
    Va = pc.align_signs(V[:, :want], Vref[:, :want])
    figs = pc.assert_backward(G[f], Va, lam[:want], lref[:want], what)
    assert pc.sign_convention_holds(V, want), what
    cons = pc.assert_consistency(B, V, lam, H[f], want, what)
    par = pc.assert_coefficients(B, Bref, parity, what) if len(parity) else 0.0
    return figs + (cons, par, int(sweeps))


def report(name, rows):
    rows = np.array(rows, dtype=np.float64)
    print(f"{name}: residual {rows[:, 0].max():.2e}, orthogonality {rows[:, 1].max():.2e}, eigenvalues "
          f"{rows[:, 2].max():.2e}, consistency {rows[:, 3].max():.2f} of its bound, parity {rows[:, 4].max():.2e}, "
          f"sweeps {int(rows[:, 5].min())}..{int(rows[:, 5].max())}")


@pytest.mark.parametrize("M", pc.GRID_M)
@pytest.mark.parametrize("K", pc.GRID_K)
def test_shape_grid(pmod, K, M):
    """(1) A single element, a single rotation, odd K (the bye), K one past every power of two and wave
    boundary: four distinct Wishart folds."""
    F, A = 4, min(K, 8)
    G, H = stack(np.random.default_rng(1000 * K + M), pc.wishart, F, K, M)
    out = fit_np(pmod, G, H, A)
    B, lam, V, nf, sweeps = out
    assert B.shape == (F, A, K, M) and lam.shape == (F, A) and V.shape == (F, K, A) and nf.shape == sweeps.shape == (F,)
    assert B.dtype == V.dtype == lam.dtype == np.float64 and nf.dtype == sweeps.dtype == np.int32
    report(f"grid K={K} M={M} 60Ku={pc.backward_bound(K):.2e}",
           [check_fold(G, H, A, out, f, f"grid K={K} M={M} fold {f}") for f in range(F)])


@pytest.mark.parametrize("K", pc.GRADED_K)
def test_graded_spectra(pmod, K):
    """(2) Spectrum 2^-j: every split is well separated, so the coefficients are held to the parity bar."""
    F, A, M = 3, min(K, 8), 3
    G, H = stack(np.random.default_rng(K), lambda r, k: pc.graded(r, k, 2), F, K, M)
    out = fit_np(pmod, G, H, A)
    report(f"graded K={K}", [check_fold(G, H, A, out, f, f"graded K={K} fold {f}", parity=range(A)) for f in range(F)])


def test_upper_limit(pmod):
    """(3) K = 512, the largest order the header allows."""
    K, F, A, M = pmod.MAX_K, 2, 16, 2
    assert K == 512
    G, H = stack(np.random.default_rng(512), pc.wishart, F, K, M)
    out = fit_np(pmod, G, H, A)
    report(f"K=512 60Ku={pc.backward_bound(K):.2e}", [check_fold(G, H, A, out, f, f"K=512 fold {f}") for f in range(F)])


def test_rank_deficiency(pmod):
    """(4) Three rows at K = 33; an all-zero matrix; the identity."""
    K, A, M = 33, 8, 2
    rng = np.random.default_rng(33)
    G = np.stack([pc.low_rank(rng, K, 3), np.zeros((K, K)), np.eye(K), pc.wishart(rng, K)])
    H = np.stack([pc.responses(rng, K, M) for _ in range(4)])
    out = fit_np(pmod, G, H, A)
    B, lam, V, nf, sweeps = out
    assert nf.tolist() == [3, 0, A, A], nf
    rows = [check_fold(G, H, A, out, 0, "three rows", n_fit=3), check_fold(G, H, A, out, 3, "wishart next to them")]
    assert not np.any(V[0][:, 3:])
    for a in range(3, A):
        assert same_bits(B[0, a], B[0, 2]), a
    assert np.all(np.abs(lam[0, 3:]) <= pc.default_rank_tol(K) * lam[0, 0]), lam[0]
    # all zero: no component, B zero, nothing NaN
    assert not np.any(B[1]) and not np.any(V[1]) and not np.any(lam[1]) and sweeps[1] == 1
    assert all(np.all(np.isfinite(t[1])) for t in out)
    # the identity: no rotation, the unit vectors in index order
    assert sweeps[2] == 1 and np.array_equal(V[2], np.eye(K)[:, :A]) and np.array_equal(lam[2], np.ones(A))
    for a in range(A):
        want = np.zeros((K, M))
        want[:a + 1] = H[2][:a + 1]
        assert np.array_equal(B[2, a], want), a
    # a larger rank_tol from the caller: the third eigenvalue of the first fold no longer counts
    tol = float(0.5 * (lam[0, 1] + lam[0, 2]) / lam[0, 0])
    out2 = fit_np(pmod, G[:1], H[:1], A, rank_tol=tol)
    assert out2[3].tolist() == [2] and same_bits(out2[0][0, 1], B[0, 1]) and same_bits(out2[0][0, 7], B[0, 1])
    report("rank deficiency", rows)


@pytest.mark.parametrize("K", pc.CLUSTER_K)
def test_clusters(pmod, K):
    """(5) Spectrum (9, 4, 4, 4, 1, ...): the backward gates on all four components (any basis of the cluster
    passes them); the coefficients where the split does not cut the cluster, a = 0 and a = 3."""
    F, A, M = 3, 4, 2
    G, H = stack(np.random.default_rng(7 * K), pc.clustered, F, K, M)
    out = fit_np(pmod, G, H, A)
    report(f"clustered K={K}", [check_fold(G, H, A, out, f, f"clustered K={K} fold {f}", parity=(0, 3)) for f in range(F)])


@pytest.mark.parametrize("case", ["nan in XTX", "inf in XTY"])
def test_non_finite_fold(pmod, case):
    """(6) The faulty fold is NaN throughout with n_fit -1 and sweeps 0; every other fold has the bits it has
    when that fold is clean."""
    K, A, M, F = 33, 6, 3, 5
    G, H = stack(np.random.default_rng(66), pc.wishart, F, K, M)
    clean = fit_np(pmod, G, H, A)
    Gd, Hd = G.copy(), H.copy()
    if case == "nan in XTX":
        bad = 2
        Gd[bad, 20, 5] = Gd[bad, 5, 20] = np.nan
    else:
        bad = 0
        Hd[bad, K - 1, M - 1] = np.inf
    out = fit_np(pmod, Gd, Hd, A)
    B, lam, V, nf, sweeps = out
    assert np.all(np.isnan(B[bad])) and np.all(np.isnan(lam[bad])) and np.all(np.isnan(V[bad]))
    assert nf[bad] == -1 and sweeps[bad] == 0
    keep = [f for f in range(F) if f != bad]
    assert np.all(nf[keep] == A) and np.all(sweeps[keep] >= 1)
    for got, ref in zip(out, clean):
        assert same_bits(got[keep], ref[keep])
    # check=True is about convergence alone: a NaN fold does not raise
    pmod.pcr_fit_batched(dev(Gd), dev(Hd), A, check=True)


def cabi_fit(G, H, A, slots=None, short=0, ws_fill=None):
    """cvm_pcr_fit through the C ABI with a workspace of `slots` slots (None: what cvm_pcr_workspace_bytes
    asks for) less `short` bytes, every byte of it `ws_fill` beforehand.  Returns (rc, outputs)."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = H.shape
    one = lib.cvm_pcr_workspace_bytes(1, K, M, A)
    nbytes = (lib.cvm_pcr_workspace_bytes(F, K, M, A) if slots is None else slots * one) - short
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    B = torch.empty((F, A, K, M), dtype=G.dtype, device="cuda")
    lam = torch.empty((F, A), dtype=torch.float64, device="cuda")
    V = torch.empty((F, K, A), dtype=G.dtype, device="cuda")
    nf = torch.empty((F,), dtype=torch.int32, device="cuda")
    sw = torch.empty((F,), dtype=torch.int32, device="cuda")
    code = _lib.CVM_F64 if G.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_pcr_fit(G.data_ptr(), H.data_ptr(), F, K, M, A, code, ctypes.c_double(0.0), B.data_ptr(), lam.data_ptr(),
                         V.data_ptr(), nf.data_ptr(), sw.data_ptr(), ws.data_ptr(), nbytes,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (B, lam, V, nf, sw))


def test_independence_and_determinism(pmod):
    """(7) A fold's bits depend on its own matrices alone."""
    from cvmatrix_amd import _lib
    K, A, M = 7, 5, 2
    rng = np.random.default_rng(77)
    G, H = stack(rng, pc.wishart, 6, K, M)
    # one fold first, last and alone
    alone = fit_np(pmod, G[:1], H[:1], A)
    first = fit_np(pmod, G, H, A)
    order = [1, 2, 3, 4, 5, 0]
    last = fit_np(pmod, G[order], H[order], A)
    for x, y, z in zip(alone, first, last):
        assert same_bits(x[0], y[0]) and same_bits(x[0], z[5])
    # more folds than workgroups, against the same folds in batches of one; the whole call twice
    F = 600
    Gb, Hb = stack(rng, pc.wishart, F, K, M)
    big = fit_np(pmod, Gb, Hb, A)
    assert same_fit(big, fit_np(pmod, Gb, Hb, A))
    assert np.all(big[3] == A) and np.all(big[4] >= 1)
    for f in (0, 1, 255, 256, 511, 512, 513, 599):
        one = fit_np(pmod, Gb[f:f + 1], Hb[f:f + 1], A)
        for x, y in zip(big, one):
            assert same_bits(x[f], y[0]), f
    for f in (3, 300, 580):                            # (the other folds: the gates, so none is another's answer)
        check_fold(Gb, Hb, A, big, f, f"fold {f} of 600")
    # a workspace of exactly one slot against the recommended one, whatever the workspace held
    Gd, Hd = dev(Gb[:40]), dev(Hb[:40])
    rc0, full = cabi_fit(Gd, Hd, A, ws_fill=0xFF)
    rc1, single = cabi_fit(Gd, Hd, A, slots=1, ws_fill=0x00)
    rc2, three = cabi_fit(Gd, Hd, A, slots=3, ws_fill=0x7F)
    assert rc0 == rc1 == rc2 == 0
    assert same_fit(full, single) and same_fit(full, three)
    assert same_fit(full, tuple(t[:40] for t in big))
    # one byte short of a slot
    rc, _ = cabi_fit(Gd, Hd, A, slots=1, short=1)
    assert rc == _lib.CVM_EWORKSPACE and b"workspace too small" in _lib.load().cvm_last_error()


def test_argument_errors(pmod):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    K, M, F, A = 8, 2, 2, 3
    G = torch.eye(K, dtype=torch.float64, device="cuda").expand(F, K, K).contiguous()
    H = torch.ones((F, K, M), dtype=torch.float64, device="cuda")
    for kw in ({"A": 0}, {"A": K + 1}, {"A": 2.0}, {"rank_tol": 1.0}, {"rank_tol": float("nan")}):
        with pytest.raises(ValueError):
            pmod.pcr_fit_batched(G, H, kw.get("A", A), rank_tol=kw.get("rank_tol"))
    with pytest.raises(ValueError):
        pmod.pcr_fit_batched(G, H.float(), A)
    with pytest.raises(ValueError):
        pmod.pcr_fit_batched(G, H[:, :5], A)
    with pytest.raises(ValueError):
        pmod.pcr_fit_batched(torch.zeros((1, 513, 513), device="cuda"), None, 1)
    B = torch.empty((F, A, K, M), dtype=torch.float64, device="cuda")
    lam = torch.empty((F, A), dtype=torch.float64, device="cuda")
    nf = torch.empty((F,), dtype=torch.int32, device="cuda")
    sw = torch.empty((F,), dtype=torch.int32, device="cuda")
    one = lib.cvm_pcr_workspace_bytes(1, K, M, A)
    ws = torch.empty(one, dtype=torch.uint8, device="cuda")

    def call(K_=K, M_=M, A_=A, dtype=_lib.CVM_F64, tol=0.0, Hp=H.data_ptr(), Bp=B.data_ptr(), lp=lam.data_ptr()):
        return lib.cvm_pcr_fit(G.data_ptr(), Hp, F, K_, M_, A_, dtype, tol, Bp, lp, None, nf.data_ptr(), sw.data_ptr(),
                               ws.data_ptr(), one, None)

    for kwargs, text in (({"lp": None}, b"null pointer"), ({"K_": 513}, b"bad shape"), ({"A_": K + 1}, b"bad shape"),
                         ({"A_": 0}, b"bad shape"), ({"M_": 65}, b"bad shape"), ({"Bp": None}, b"PCA only"),
                         ({"M_": 0}, b"PCA only"), ({"tol": 1.0}, b"rank_tol"), ({"tol": float("nan")}, b"rank_tol"),
                         ({"dtype": 7}, b"dtype")):
        assert call(**kwargs) == _lib.CVM_EINVAL, kwargs
        assert text in lib.cvm_last_error(), (kwargs, lib.cvm_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    assert nf.tolist() == [A, A] and sw.tolist() == [1, 1]
    # F = 0: empty tensors, nothing launched; a single (K, K) with (K,)
    empty = pmod.pcr_fit_batched(G[:0], H[:0], A, return_components=True, check=True)
    assert empty.B.shape == (0, A, K, M) and empty.eigenvalues.shape == (0, A) and empty.components.shape == (0, K, A)
    assert empty.n_fit.shape == empty.sweeps.shape == (0,)
    single = pmod.pcr_fit_batched(G[0], H[0, :, 0], A)
    assert single.B.shape == (1, A, K, 1) and single.components is None


def test_float32(pmod):
    """(8) float32 in and out: one float32 rounding on top of the float64 gates; the reference is computed from
    the widened inputs."""
    from cvmatrix_amd import CVMatrix
    rng = np.random.default_rng(3)
    N, K, M, P, A = 3000, 64, 3, 5, 6
    X = rng.standard_normal((N, K)).astype(np.float32) * np.linspace(1.0, 4.0, K, dtype=np.float32)
    Y = rng.standard_normal((N, M)).astype(np.float32)
    cvm = CVMatrix(True, True, False, False, dtype=np.float32)
    cvm.fit(X, Y)
    (XTX, XTY), _ = cvm.training_XTX_XTY_batched(cvm.prepare_folds([np.arange(N)[np.arange(N) % P == f] for f in range(P)]))
    assert XTX.dtype == torch.float32
    fit = pmod.pcr_fit_batched(XTX, XTY, A, return_components=True)
    assert fit.B.dtype == torch.float32 and fit.components.dtype == torch.float32 and fit.eigenvalues.dtype == torch.float64
    G, H = XTX.double().cpu().numpy(), XTY.double().cpu().numpy()
    B, lam, V = fit.B.cpu().numpy(), fit.eigenvalues.cpu().numpy(), fit.components.double().cpu().numpy()
    assert fit.n_fit.tolist() == [A] * P
    worst = 0.0
    for f in range(P):
        Bref, lref, Vref, _ = pc.pcr_reference(G[f], H[f], A)
        # (the columns of X have standard deviations from 1 to 4: the leading eigenvalues are well apart)
        worst = max(worst, pc.assert_coefficients(B[f], Bref, range(A), f"float32 fold {f}", float32=True))
        assert np.max(np.abs(lam[f] - lref)) <= pc.backward_bound(K) * np.linalg.norm(G[f])
        Va = pc.align_signs(V[f], Vref)
        assert np.linalg.norm(Va.T @ Va - np.eye(A)) <= (pc.backward_bound(K) + 2 * pc.F32_STORE) * np.sqrt(A)
    print(f"float32: B within {worst:.2e} of the reference (gate {pc.PARITY + pc.F32_STORE:.2e})")


def test_pca_only(pmod):
    """(9) XTY=None: B is None, components and eigenvalues as in the same call with XTY."""
    K, A, M, F = 33, 5, 2, 3
    G, H = stack(np.random.default_rng(9), pc.wishart, F, K, M)
    both = pmod.pcr_fit_batched(dev(G), dev(H), A, return_components=True)
    pca = pmod.pcr_fit_batched(dev(G), None, A)
    assert pca.B is None and pca.components is not None
    for x, y in zip(both[1:], pca[1:]):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    one = pmod.pcr_fit_batched(dev(G[1]), None, A)
    assert same_bits(one.components[0].cpu().numpy(), pca.components[1].cpu().numpy())


def refit_predictions(X, Y, w, val, A):
    """PCR refitted from scratch in NumPy on the training rows (weighted means, weighted cross products);
    predictions on the validation rows for 1 .. A components."""
    tr = np.setdiff1d(np.arange(X.shape[0]), val)
    wt = w[tr]
    mx, my = (wt @ X[tr]) / wt.sum(), (wt @ Y[tr]) / wt.sum()
    Xs, Ys = X[tr] - mx, Y[tr] - my
    B, *_ = pc.pcr_reference(Xs.T @ (wt[:, None] * Xs), Xs.T @ (wt[:, None] * Ys), A)
    return np.einsum("nk,akm->anm", X[val] - mx, B) + my


def test_end_to_end_against_refits(pmod):
    """(10) CVMatrix -> training_XTX_XTY_batched -> pcr_fit_batched -> pls_validation_sse -> cv_rmse against
    PCR refitted on every training set in NumPy.  The columns of X have graded scales, so the leading
    eigenvalues are well apart and the first A components are defined to the conditioning of the refit
    test of the device ridge: predictions and SSE to 1e-9 relative."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import cv_rmse, pls_validation_sse
    rng = np.random.default_rng(10)
    N, K, M, P, A = 600, 24, 2, 5, 6
    X = rng.standard_normal((N, K)) * (1.5 ** -np.arange(K)) * 4.0 + 0.5
    Y = X[:, :4] @ rng.standard_normal((4, M)) + 0.3 * rng.standard_normal((N, M)) + 1.0
    w = rng.random(N) + 0.1
    labels = rng.integers(0, P, N)
    p = amd.Partitioner(labels)
    cvm = amd.CVMatrix(True, True, False, False, dtype=np.float64, copy=False)
    cvm.fit(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(w).cuda())
    batch = cvm.prepare_folds(p)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    fit = pmod.pcr_fit_batched(XTX, XTY, A, check=True)
    assert fit.n_fit.tolist() == [A] * P
    sse, wsum = pls_validation_sse(cvm, batch, stats, fit.B)
    rmse = cv_rmse(sse, wsum).cpu().numpy()
    sse = sse.cpu().numpy()
    B = fit.B.cpu().numpy()
    muX, muY = stats[0].cpu().numpy(), stats[2].cpu().numpy()
    total = np.zeros((A, M))
    for f, key in enumerate(p.folds_dict):
        val = p.get_validation_indices(key)
        ref = refit_predictions(X, Y, w, val, A)
        got = np.einsum("nk,akm->anm", X[val] - muX[f], B[f]) + muY[f]
        assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (f, np.abs(got - ref).max())
        ref_sse = np.einsum("n,anm->am", w[val], (ref - Y[val]) ** 2)
        np.testing.assert_allclose(sse[f], ref_sse, rtol=1e-9)
        total += ref_sse
    np.testing.assert_allclose(rmse, np.sqrt(total / w.sum()), rtol=1e-9)
