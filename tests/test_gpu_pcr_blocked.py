"""GPU (-m gpu): the blocked device eigensolver (cvm_pcr_blocked_fit through pcr_fit_batched(solver="blocked") and
the C ABI) against the reference, the designs and the gates of tests/pcr_cases.py, at the shapes of
tests/pcr_blocked_cases.py (b = pcr.BLOCK).  The gates are the scalar solver's, not widened; every test prints
where the kernel lands (run with -s).  On the MI355X, the largest figure over the folds of a test (residual,
orthogonality, eigenvalues, each against 60 K u; sweeps):
  test_block_boundary_grid  K = 32    9.4e-16  6.5e-15  5.6e-16  against 2.1e-13   8..9 sweeps
                            K = 65    1.4e-15  2.0e-14  6.0e-16  against 4.3e-13   7..8 sweeps
                            K = 163   2.0e-15  5.8e-14  6.5e-16  against 1.1e-12   9 sweeps
  test_graded_spectra       K = 33    1.2e-15  7.4e-15  3.4e-16  against 2.2e-13   13..14 sweeps
                            K = 129   5.1e-15  1.1e-13  2.5e-15  against 8.6e-13   15..16 sweeps (the most seen)
                            K = 257   1.3e-14  1.7e-13  8.0e-15  against 1.7e-12   14..15 sweeps
  test_clusters             K = 129   2.6e-15  9.2e-15  1.7e-15  against 8.6e-13   5..6 sweeps
  test_past_the_old_limit   K = 513   4.7e-15  2.6e-13  6.1e-16  against 3.4e-12   12 sweeps
                            K = 640   3.6e-15  3.2e-13  6.5e-16  against 4.3e-12   12 sweeps
                            K = 1024  6.2e-15  6.0e-13  9.3e-16  against 6.8e-12   13 sweeps, 0.5 s
  test_upper_limit          K = 4096  1.2e-14  3.3e-12  1.3e-15  against 2.7e-11   14 sweeps, 0.61 s for the fit (1.3 s
                                                                                   with torch.linalg.eigvalsh)
Coefficients against the reference (gate 1e-10): graded at most 4.0e-13 (K = 257), clustered a = 0, 3 at most
1.0e-14; float32 3.8e-8 against 1e-10 + 2^-24 = 6.0e-8.  Consistency: below 0.005 of its bound in every test.  The two
solvers: eigenvalues within 3.7e-15 ||G||_F, coefficients within 1.9e-13 (K = 129).  test_bit_contract: the six folds
take 8, 7, 7, 5, 5 and 3 sweeps."""

import ctypes

import numpy as np
import pytest
import torch

import pcr_blocked_cases as bc
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


def fit_np(pmod, G, H, A, solver="blocked", **kw):
    """pcr_fit_batched on NumPy stacks; everything back as NumPy."""
    fit = pmod.pcr_fit_batched(dev(G), None if H is None else dev(H), A, return_components=True, solver=solver, **kw)
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
    parity on the components in `parity`.  Returns the figures.  (check_fold of tests/test_gpu_pcr.py, restated.)"""
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


@pytest.mark.parametrize("M", bc.GRID_M)
@pytest.mark.parametrize("K", bc.grid_K(32))
def test_block_boundary_grid(pmod, K, M):
    """(1) One block, one exact pair, a ragged last block of one column, an odd number of blocks (the padding
    block as a partner), padding: four distinct Wishart folds."""
    assert pmod.BLOCK == 32                           # (the parameters above are written out for it)
    F, A = 4, min(K, 8)
    G, H = stack(np.random.default_rng(1000 * K + M), pc.wishart, F, K, M)
    out = fit_np(pmod, G, H, A)
    B, lam, V, nf, sweeps = out
    assert B.shape == (F, A, K, M) and lam.shape == (F, A) and V.shape == (F, K, A) and nf.shape == sweeps.shape == (F,)
    assert B.dtype == V.dtype == lam.dtype == np.float64 and nf.dtype == sweeps.dtype == np.int32
    report(f"grid K={K} M={M} 60Ku={pc.backward_bound(K):.2e}",
           [check_fold(G, H, A, out, f, f"grid K={K} M={M} fold {f}") for f in range(F)])


@pytest.mark.parametrize("K", bc.graded_K(32))
def test_graded_spectra(pmod, K):
    """(2) Spectrum 2^-j: every split is well separated, so the coefficients are held to the parity bar."""
    F, A, M = 3, 8, 3
    G, H = stack(np.random.default_rng(K), lambda r, k: pc.graded(r, k, 2), F, K, M)
    out = fit_np(pmod, G, H, A)
    report(f"graded K={K}", [check_fold(G, H, A, out, f, f"graded K={K} fold {f}", parity=range(A)) for f in range(F)])


def test_clusters(pmod):
    """(3) Spectrum (9, 4, 4, 4, 1, ...) at K = 129: the coefficients at a = 0 and a = 3."""
    K, F, A, M = 129, 3, 4, 2
    G, H = stack(np.random.default_rng(7 * K), pc.clustered, F, K, M)
    out = fit_np(pmod, G, H, A)
    report(f"clustered K={K}", [check_fold(G, H, A, out, f, f"clustered K={K} fold {f}", parity=(0, 3)) for f in range(F)])


@pytest.mark.parametrize("K,F,A,M", bc.PAST_OLD_LIMIT)
def test_past_the_old_limit(pmod, K, F, A, M):
    """(4) K = 513, 640, 1024: Wishart designs against numpy.linalg.eigh, all gates."""
    assert K > pmod.MAX_K
    G, H = stack(np.random.default_rng(K), pc.wishart, F, K, M)
    out = fit_np(pmod, G, H, A)
    assert np.all(out[4] >= 1) and np.all(out[4] <= 60)
    report(f"K={K} 60Ku={pc.backward_bound(K):.2e}", [check_fold(G, H, A, out, f, f"K={K} fold {f}") for f in range(F)])


def test_upper_limit(pmod):
    """(5) K = 4096, one Wishart fold generated on the device; residual, orthogonality and eigenvalues (against
    torch.linalg.eigvalsh) computed on the device in float64, each against 60 K u."""
    import time
    K, A, M = pmod.MAX_K_BLOCKED, 16, 1
    assert K == 4096
    gen = torch.Generator(device="cuda").manual_seed(4096)
    X = torch.randn((2 * K + 3, K), dtype=torch.float64, device="cuda", generator=gen)
    G = X.T @ X
    G = 0.5 * (G + G.T)
    H = torch.randn((K, M), dtype=torch.float64, device="cuda", generator=gen)
    del X
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = pmod.pcr_fit_batched(G[None], H[None], A, return_components=True, solver="blocked")
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert fit.n_fit.tolist() == [A] and 1 <= int(fit.sweeps[0]) <= 60
    lam, V = fit.eigenvalues[0], fit.components[0]
    nG = torch.linalg.norm(G)
    res = float(torch.linalg.norm(G @ V - V * lam) / nG)
    orth = float(torch.linalg.norm(V.T @ V - torch.eye(A, dtype=torch.float64, device="cuda"))) / np.sqrt(A)
    lref = torch.linalg.eigvalsh(G).flip(0)[:A]
    eig = float((lam - lref).abs().max() / nG)
    bound = pc.backward_bound(K)
    print(f"K=4096: residual {res:.2e}, orthogonality {orth:.2e}, eigenvalues {eig:.2e} against {bound:.2e}, "
          f"{int(fit.sweeps[0])} sweeps, {seconds:.2f} s")
    assert res <= bound and orth <= bound and eig <= bound
    assert bool(torch.all(lam[:-1] >= lam[1:]))
    Vh = V.cpu().numpy()
    assert pc.sign_convention_holds(Vh, A)
    # the coefficients against the formula on the fit's own components, on the device
    want = torch.cumsum(torch.einsum("ka,am->akm", V, (V.T @ H) / lam[:, None]), dim=0)
    assert float(torch.linalg.norm(fit.B[0] - want) / torch.linalg.norm(want)) <= 1e-10


def test_rank_and_trivial_matrices(pmod):
    """(6) Three rows, the zero matrix, the identity and a Wishart fold at K = 2b + 1."""
    K, A, M = 2 * pmod.BLOCK + 1, 8, 2
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
    assert not np.any(B[1]) and not np.any(V[1]) and not np.any(lam[1]) and sweeps[1] == 1
    assert all(np.all(np.isfinite(t[1])) for t in out)
    assert sweeps[2] == 1 and np.array_equal(V[2], np.eye(K)[:, :A]) and np.array_equal(lam[2], np.ones(A))
    for a in range(A):
        want = np.zeros((K, M))
        want[:a + 1] = H[2][:a + 1]
        assert np.array_equal(B[2, a], want), a
    report("rank and trivial matrices", rows)


def test_non_finite_folds(pmod):
    """(7) Five folds at K = 65: fold 1 with a NaN in XTX, fold 3 with an infinity in XTY."""
    K, A, M, F = 65, 6, 3, 5
    G, H = stack(np.random.default_rng(66), pc.wishart, F, K, M)
    keep = [0, 2, 4]
    clean = fit_np(pmod, G[keep], H[keep], A)
    Gd, Hd = G.copy(), H.copy()
    Gd[1, 40, 5] = Gd[1, 5, 40] = np.nan
    Hd[3, K - 1, M - 1] = np.inf
    out = fit_np(pmod, Gd, Hd, A)
    B, lam, V, nf, sweeps = out
    for bad in (1, 3):
        assert np.all(np.isnan(B[bad])) and np.all(np.isnan(lam[bad])) and np.all(np.isnan(V[bad]))
        assert nf[bad] == -1 and sweeps[bad] == 0
    assert np.all(nf[keep] == A) and np.all(sweeps[keep] >= 1)
    for got, ref in zip(out, clean):
        assert same_bits(got[keep], ref)
    pmod.pcr_fit_batched(dev(Gd), dev(Hd), A, check=True, solver="blocked")      # (a NaN fold does not raise)


def cabi_fit(G, H, A, slots=None, short=0, ws_fill=None, max_sweeps=60):
    """cvm_pcr_blocked_fit through the C ABI with a workspace of `slots` slots (None: what
    cvm_pcr_blocked_workspace_bytes asks for) less `short` bytes, filled with the float64 `ws_fill` beforehand."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = H.shape
    one = lib.cvm_pcr_blocked_workspace_bytes(1, K, M, A)
    nbytes = (lib.cvm_pcr_blocked_workspace_bytes(F, K, M, A) if slots is None else slots * one) - short
    ws = torch.empty(max(nbytes, 8) // 8 + 1, dtype=torch.float64, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    B = torch.empty((F, A, K, M), dtype=G.dtype, device="cuda")
    lam = torch.empty((F, A), dtype=torch.float64, device="cuda")
    V = torch.empty((F, K, A), dtype=G.dtype, device="cuda")
    nf = torch.empty((F,), dtype=torch.int32, device="cuda")
    sw = torch.empty((F,), dtype=torch.int32, device="cuda")
    code = _lib.CVM_F64 if G.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_pcr_blocked_fit(G.data_ptr(), H.data_ptr(), F, K, M, A, code, ctypes.c_double(0.0), max_sweeps,
                                 B.data_ptr(), lam.data_ptr(), V.data_ptr(), nf.data_ptr(), sw.data_ptr(),
                                 ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (B, lam, V, nf, sw))


SCALES = (1.0, 1.02, 1.05, 1.1, 1.2, 1.5)


def scaled_wishart(rng, K, ratio, made):
    """X^T X with column j of X scaled by ratio^-j: from a flat Wishart spectrum to one graded over 34 decades."""
    made.append(ratio)
    X = rng.standard_normal((2 * K + 3, K)) * float(ratio) ** -np.arange(K)
    return pc.sym(X.T @ X)


def test_bit_contract(pmod):
    """(8) A fold's bits depend on its own matrices alone: six Wishart folds at K = 97 whose spectra have
    different scales (they finish in different sweeps) as a batch, alone, reversed, with one and two slots, over a
    workspace full of NaN, and twice."""
    from cvmatrix_amd import _lib
    K, A, M, F = 97, 5, 2, 6
    rng = np.random.default_rng(97)
    made = []
    G, H = stack(rng, lambda r, k: scaled_wishart(r, k, SCALES[len(made)], made), F, K, M)
    Gd, Hd = dev(G), dev(H)
    rc, full = cabi_fit(Gd, Hd, A)
    assert rc == 0
    assert len(set(full[4].tolist())) >= 2, full[4]   # (the folds do drop out at different sweeps)
    for f in range(F):
        check_fold(G, H, A, full, f, f"bit contract fold {f}")
    rc, again = cabi_fit(Gd, Hd, A)
    assert rc == 0 and same_fit(full, again)
    for f in range(F):
        rc, one = cabi_fit(Gd[f:f + 1].contiguous(), Hd[f:f + 1].contiguous(), A)
        assert rc == 0
        for x, y in zip(full, one):
            assert same_bits(x[f], y[0]), f
    rc, rev = cabi_fit(Gd.flip(0).contiguous(), Hd.flip(0).contiguous(), A)
    assert rc == 0 and same_fit(full, tuple(t[::-1] for t in rev))
    rc1, single = cabi_fit(Gd, Hd, A, slots=1, ws_fill=0.0)
    rc2, two = cabi_fit(Gd, Hd, A, slots=2, ws_fill=1.0)
    rc3, nans = cabi_fit(Gd, Hd, A, ws_fill=float("nan"))
    assert rc1 == rc2 == rc3 == 0
    assert same_fit(full, single) and same_fit(full, two) and same_fit(full, nans)
    rc, _ = cabi_fit(Gd, Hd, A, slots=1, short=1)
    assert rc == _lib.CVM_EWORKSPACE and b"workspace too small" in _lib.load().cvm_last_error()
    print(f"bit contract: sweeps {full[4].tolist()}")


def test_max_sweeps(pmod):
    """(9) One sweep is not enough for a Wishart fold at K = 129 (the model needs 9); the identity beside it is
    done after one."""
    K, A, M = 129, 4, 2
    rng = np.random.default_rng(129)
    G = np.stack([pc.wishart(rng, K), np.eye(K)])
    H = np.stack([pc.responses(rng, K, M) for _ in range(2)])
    B, lam, V, nf, sweeps = fit_np(pmod, G, H, A, max_sweeps=1)
    assert sweeps.tolist() == [-1, 1] and nf.tolist() == [-1, A]
    assert np.all(np.isnan(B[0])) and np.all(np.isnan(lam[0])) and np.all(np.isnan(V[0]))
    assert np.array_equal(V[1], np.eye(K)[:, :A]) and np.array_equal(lam[1], np.ones(A)) and np.all(np.isfinite(B[1]))
    with pytest.raises(np.linalg.LinAlgError, match="fold 0"):
        pmod.pcr_fit_batched(dev(G), dev(H), A, solver="blocked", max_sweeps=1, check=True)
    full = fit_np(pmod, G, H, A)
    assert full[4][0] > 1 and full[4][1] == 1
    print(f"max_sweeps: the Wishart fold takes {int(full[4][0])} sweeps")


def test_float32(pmod):
    """(10) float32 in and out, as tests/test_gpu_pcr.py builds the folds, at K = 65."""
    from cvmatrix_amd import CVMatrix
    rng = np.random.default_rng(3)
    N, K, M, P, A = 3000, 65, 3, 5, 6
    X = rng.standard_normal((N, K)).astype(np.float32) * np.linspace(1.0, 4.0, K, dtype=np.float32)
    Y = rng.standard_normal((N, M)).astype(np.float32)
    cvm = CVMatrix(True, True, False, False, dtype=np.float32)
    cvm.fit(X, Y)
    (XTX, XTY), _ = cvm.training_XTX_XTY_batched(cvm.prepare_folds([np.arange(N)[np.arange(N) % P == f] for f in range(P)]))
    assert XTX.dtype == torch.float32
    fit = pmod.pcr_fit_batched(XTX, XTY, A, return_components=True, solver="blocked")
    assert fit.B.dtype == torch.float32 and fit.components.dtype == torch.float32 and fit.eigenvalues.dtype == torch.float64
    G, H = XTX.double().cpu().numpy(), XTY.double().cpu().numpy()
    B, lam, V = fit.B.cpu().numpy(), fit.eigenvalues.cpu().numpy(), fit.components.double().cpu().numpy()
    assert fit.n_fit.tolist() == [A] * P
    worst = 0.0
    for f in range(P):
        Bref, lref, Vref, _ = pc.pcr_reference(G[f], H[f], A)
        worst = max(worst, pc.assert_coefficients(B[f], Bref, range(A), f"float32 fold {f}", float32=True))
        assert np.max(np.abs(lam[f] - lref)) <= pc.backward_bound(K) * np.linalg.norm(G[f])
        Va = pc.align_signs(V[f], Vref)
        assert np.linalg.norm(Va.T @ Va - np.eye(A)) <= (pc.backward_bound(K) + 2 * pc.F32_STORE) * np.sqrt(A)
    print(f"float32: B within {worst:.2e} of the reference (gate {pc.PARITY + pc.F32_STORE:.2e})")


@pytest.mark.parametrize("K", [33, 129])
def test_the_two_solvers_agree(pmod, K):
    """(11) The same call through both solvers on a graded design; the scalar solver's bits are its own."""
    F, A, M = 3, 8, 3
    G, H = stack(np.random.default_rng(11 * K), lambda r, k: pc.graded(r, k, 2), F, K, M)
    scalar = fit_np(pmod, G, H, A, solver="scalar")
    blocked = fit_np(pmod, G, H, A)
    assert same_fit(scalar, fit_np(pmod, G, H, A, solver="scalar"))
    default = pmod.pcr_fit_batched(dev(G), dev(H), A, return_components=True)
    assert same_fit(scalar, tuple(t.cpu().numpy() for t in default))
    assert np.array_equal(scalar[3], blocked[3])
    worst_l = worst_b = 0.0
    for f in range(F):
        nG = np.linalg.norm(G[f])
        dl = np.max(np.abs(scalar[1][f] - blocked[1][f]))
        assert dl <= 2 * pc.backward_bound(K) * nG, (f, dl)
        worst_l = max(worst_l, dl / nG)
        for a in range(A):
            e = pc.coefficient_error(blocked[0][f, a], scalar[0][f, a])
            assert e <= 2e-10, (f, a, e)
            worst_b = max(worst_b, e)
    print(f"two solvers K={K}: eigenvalues within {worst_l:.2e} ||G||, coefficients within {worst_b:.2e}")


def test_cabi_refusals(pmod):
    """(12) CVM_EINVAL for bad pointers, shapes, rank_tol, dtype and max_sweeps; n_folds == 0 launches nothing."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    K, M, F, A = 8, 2, 2, 3
    G = torch.eye(K, dtype=torch.float64, device="cuda").expand(F, K, K).contiguous()
    H = torch.ones((F, K, M), dtype=torch.float64, device="cuda")
    B = torch.empty((F, A, K, M), dtype=torch.float64, device="cuda")
    lam = torch.empty((F, A), dtype=torch.float64, device="cuda")
    nf = torch.full((F,), 77, dtype=torch.int32, device="cuda")
    sw = torch.full((F,), 77, dtype=torch.int32, device="cuda")
    one = lib.cvm_pcr_blocked_workspace_bytes(1, K, M, A)
    ws = torch.empty(one, dtype=torch.uint8, device="cuda")

    def call(K_=K, M_=M, A_=A, F_=F, dtype=_lib.CVM_F64, tol=0.0, ms=60, Gp=G.data_ptr(), Hp=H.data_ptr(),
             Bp=B.data_ptr(), lp=lam.data_ptr(), wp=ws.data_ptr()):
        return lib.cvm_pcr_blocked_fit(Gp, Hp, F_, K_, M_, A_, dtype, tol, ms, Bp, lp, None, nf.data_ptr(), sw.data_ptr(),
                                       wp, one, None)

    for kwargs, text in (({"lp": None}, b"null pointer"), ({"Gp": None}, b"null pointer"), ({"wp": None}, b"null pointer"),
                         ({"K_": 4097}, b"bad shape"), ({"A_": K + 1}, b"bad shape"), ({"A_": 0}, b"bad shape"),
                         ({"M_": 65}, b"bad shape"), ({"Bp": None}, b"PCA only"), ({"M_": 0}, b"PCA only"),
                         ({"tol": 1.0}, b"rank_tol"), ({"tol": float("nan")}, b"rank_tol"), ({"dtype": 7}, b"dtype"),
                         ({"ms": 0}, b"max_sweeps"), ({"ms": 61}, b"max_sweeps")):
        assert call(**kwargs) == _lib.CVM_EINVAL, kwargs
        assert text in lib.cvm_last_error(), (kwargs, lib.cvm_last_error())
    assert call(F_=0) == 0
    torch.cuda.synchronize()
    assert nf.tolist() == [77, 77] and sw.tolist() == [77, 77]          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert nf.tolist() == [A, A] and sw.tolist() == [1, 1]
    # the Python side: F = 0, a single (K, K) with (K,), PCA only, the scalar solver's limit
    empty = pmod.pcr_fit_batched(G[:0], H[:0], A, return_components=True, check=True, solver="blocked")
    assert empty.B.shape == (0, A, K, M) and empty.n_fit.shape == empty.sweeps.shape == (0,)
    single = pmod.pcr_fit_batched(G[0], H[0, :, 0], A, solver="blocked")
    assert single.B.shape == (1, A, K, 1) and single.components is None
    pca = pmod.pcr_fit_batched(G, None, A, solver="blocked")
    assert pca.B is None and pca.components.shape == (F, K, A)
    with pytest.raises(ValueError):
        pmod.pcr_fit_batched(torch.zeros((1, 513, 513), device="cuda"), None, 1, solver="scalar")
