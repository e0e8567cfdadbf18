"""GPU (-m gpu): the device PCA-LDA (cvm_pcalda_fit through cvmatrix_amd/pcalda.py) against the truth and the gate
of tests/pcalda_cases.py -- err <= 2 Y + c u (float32: + 2^-24), derived there and not calibrated -- and the rules of
include/cvmhip.h: the stopping decisions, the padding, absent classes, flagged folds, and that a fold's bits depend
on its own inputs alone.  The inputs of the accuracy tests are formed by NumPy (eigh on the CPU) and uploaded to
``pcalda_from_components``, so that the device and the yardstick see the same bits.

Where the kernels land on the MI355X (CVM_PCALDA_REPORT), the largest err / Y per test: DESIGN.md 4.16."""

import numpy as np
import pytest
import torch

import lda_cases as lc
import pcalda_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pmod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import pcalda as mod
    return mod


def device_fit(pmod, V, E, nc, XTY, CW, **kw):
    """pcalda_from_components on uploaded copies; (coef, intercept, priors, n_fit, info) as NumPy arrays."""
    fit = pmod.pcalda_from_components(*(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (V, E, nc, XTY, CW)), **kw)
    return tuple(t.cpu().numpy() for t in fit[:5])


def assert_padding(coef, icpt, n_fit, CW):
    """Models a >= n_fit repeat model n_fit - 1 to the bit; n_fit 0 is the prior-only model."""
    for f in range(coef.shape[0]):
        nf = n_fit[f]
        if nf > 0:
            assert np.array_equal(coef[f, nf:], np.broadcast_to(coef[f, nf - 1], coef[f, nf:].shape)), f
            assert np.array_equal(icpt[f, nf:], np.broadcast_to(icpt[f, nf - 1], icpt[f, nf:].shape)), f
        else:
            assert not coef[f].any(), f
            want = pc.prior_only(CW[f], coef.shape[2])[1].astype(icpt.dtype)
            assert np.allclose(icpt[f], np.broadcast_to(want, icpt[f].shape), rtol=4 * pc.U, atol=0), f


@pytest.mark.parametrize("K,C,A,dtype", [(K, C, A, np.float64) for K, C, A in pc.GRID] +
                         [(K, C, A, np.float32) for K, C, A in pc.GRID_F32])
def test_shape_grid(pmod, K, C, A, dtype):
    V, E, nc, XTY, CW = pc.grid_case(K, C, A)
    V, XTY = V.astype(dtype), XTY.astype(dtype)
    ref = pc.grid_reference(K, C, A) if dtype == np.float64 else pc.Reference(V, E, nc, XTY, CW)
    coef, icpt, priors, n_fit, info = device_fit(pmod, V, E, nc, XTY, CW)
    assert coef.shape == (3, A, K, C) and icpt.shape == (3, A, C) and coef.dtype == dtype and icpt.dtype == dtype
    assert n_fit.dtype == np.int32 and info.dtype == np.int32
    assert np.array_equal(n_fit, ref.n_fit) and np.array_equal(info, ref.info) and np.all(n_fit == A) and not info.any()
    assert priors.dtype == np.float64 and np.array_equal(priors, CW / CW.sum(axis=1, keepdims=True))
    worst = pc.assert_gate(coef, icpt, ref, f"grid K={K} C={C} A={A} {np.dtype(dtype).name}", float32=dtype == np.float32)
    print(f"K={K} C={C} A={A} {np.dtype(dtype).name}: largest err / Y {worst:.3f}")


@pytest.mark.parametrize("sep", pc.LADDER_SEP)
def test_cancellation_ladder(pmod, sep):
    """Class means 1, 1e2 and 1e4 within-class standard deviations apart: the leading eigenvalues are up to 1e8
    times the pivots and the downdate loses that many digits, in the device and in the yardstick alike."""
    case = pc.ladder_case(sep)
    ref = pc.Reference(*case, pivot_tol=pc.LADDER_PIVOT_TOL)
    coef, icpt, _, n_fit, info = device_fit(pmod, *case, pivot_tol=pc.LADDER_PIVOT_TOL)
    assert np.array_equal(n_fit, ref.n_fit) and not info.any()
    worst = pc.assert_gate(coef, icpt, ref, f"ladder sep={sep:g}")
    print(f"sep={sep:g}: rho {ref.rho:.3g}, amp {ref.amp:.3g}, largest err / Y {worst:.3f}")


def test_stopping_at_a_pivot(pmod):
    """K = 40 on 30 rows, C = 3, A = 32: 27 models, info 2, the padding bit-equal to model 26; the other folds whole."""
    case = pc.stopping_pivot_case()
    ref = pc.Reference(*case)
    coef, icpt, _, n_fit, info = device_fit(pmod, *case)
    assert n_fit.tolist() == [32, 27, 32] and info.tolist() == [0, 2, 0]
    assert np.array_equal(n_fit, ref.n_fit) and np.array_equal(info, ref.info)
    assert np.all(np.isfinite(coef)) and np.all(np.isfinite(icpt))
    assert_padding(coef, icpt, n_fit, case[4])
    assert not np.array_equal(coef[1, 26], coef[1, 25])
    worst = pc.assert_gate(coef, icpt, ref, "stopping at a pivot")
    print(f"stopping at a pivot: largest err / Y {worst:.3f}")


def test_stopping_at_the_components_that_exist(pmod):
    case = pc.stopping_rank_case()
    ref = pc.Reference(*case)
    coef, icpt, _, n_fit, info = device_fit(pmod, *case)
    assert n_fit.tolist() == [10, 10, 10] and info.tolist() == [1, 1, 1]
    assert_padding(coef, icpt, n_fit, case[4])
    worst = pc.assert_gate(coef, icpt, ref, "stopping at n_comp")
    print(f"stopping at n_comp: largest err / Y {worst:.3f}")
    # n_comp = 0: the prior-only model, info 1
    V, E, nc, XTY, CW = (t.copy() for t in case)
    nc[1] = 0
    coef0, icpt0, _, n_fit0, info0 = device_fit(pmod, V, E, nc, XTY, CW)
    assert n_fit0.tolist() == [10, 0, 10] and info0.tolist() == [1, 1, 1]
    assert_padding(coef0, icpt0, n_fit0, CW)
    assert np.array_equal(coef0[[0, 2]], coef[[0, 2]]) and np.array_equal(icpt0[[0, 2]], icpt[[0, 2]])


def test_separated_classes_give_the_prior_only_model(pmod):
    case = pc.separated_case()
    ref = pc.Reference(*case)
    coef, icpt, priors, n_fit, info = device_fit(pmod, *case)
    assert n_fit.tolist() == [4, 0, 4] and info.tolist() == [0, 2, 0]
    assert_padding(coef, icpt, n_fit, case[4])
    assert np.allclose(icpt[1], np.log(priors[1])[None], rtol=4 * pc.U, atol=0)
    pc.assert_gate(coef, icpt, ref, "separated classes")


def test_absent_class(pmod):
    """Fold 1 trains without class 2: coef 0, intercept -inf and priors 0 for that class there; the other classes
    pass the gate; the other folds have the bits they have when run without fold 1."""
    case = pc.absent_case()
    ref = pc.Reference(*case)
    coef, icpt, priors, n_fit, info = device_fit(pmod, *case)
    assert not info.any() and np.all(n_fit == 12)
    assert not coef[1, :, :, 2].any() and np.all(np.isneginf(icpt[1, :, 2])) and priors[1, 2] == 0.0
    assert np.all(np.isfinite(np.delete(icpt, 2, axis=2))) and np.all(np.isfinite(icpt[[0, 2]]))
    assert np.all(np.isfinite(coef)) and np.all(priors[[0, 2]] > 0)
    worst = pc.assert_gate(coef, icpt, ref, "absent class")
    print(f"absent class: largest err / Y {worst:.3f}")
    others = device_fit(pmod, *(t[[0, 2]] for t in case))
    assert np.array_equal(others[0], coef[[0, 2]]) and np.array_equal(others[1], icpt[[0, 2]])


def poison(kind, V, E, nc, XTY, CW):
    """Fold 1 of copies of the batch made unusable."""
    V, E, nc, XTY, CW = (t.copy() for t in (V, E, nc, XTY, CW))
    K = V.shape[1]
    if kind == "nan in V":
        V[1, K - 1, 0] = np.nan
    elif kind == "inf in V":
        V[1, 0, V.shape[2] - 1] = np.inf
    elif kind == "nan in eig":
        E[1, 1] = np.nan
    elif kind == "inf in eig":
        E[1, 0] = np.inf
    elif kind == "nan in XTY":
        XTY[1, K // 2, 1] = np.nan
    elif kind == "inf in XTY":
        XTY[1, K - 1, 2] = -np.inf
    elif kind == "nan class weight":
        CW[1, 2] = np.nan
    elif kind == "inf class weight":
        CW[1, 0] = np.inf
    elif kind == "negative class weight":
        CW[1, 0] = -CW[1, 0]
    elif kind == "no weight":
        CW[1] = 0.0
    elif kind == "n_comp -1":
        nc[1] = -1
    return V, E, nc, XTY, CW


@pytest.mark.parametrize("kind", ["nan in V", "inf in V", "nan in eig", "inf in eig", "nan in XTY", "inf in XTY",
                                  "nan class weight", "inf class weight", "negative class weight", "no weight",
                                  "n_comp -1"])
def test_flagged_fold(pmod, kind):
    """The flagged fold has info -1, n_fit -1 and NaN in every coef and intercept; the other folds keep their bits."""
    case = pc.grid_case(33, 3, 33)
    coef, icpt, _, n_fit, info = device_fit(pmod, *case)
    bad = poison(kind, *case)
    coef_b, icpt_b, _, n_fit_b, info_b = device_fit(pmod, *bad)
    assert info_b.tolist() == [0, -1, 0] and n_fit_b.tolist() == [33, -1, 33]
    assert np.all(np.isnan(coef_b[1])) and np.all(np.isnan(icpt_b[1]))
    assert np.array_equal(coef_b[[0, 2]], coef[[0, 2]]) and np.array_equal(icpt_b[[0, 2]], icpt[[0, 2]])
    with pytest.raises(np.linalg.LinAlgError, match="fold 1"):
        device_fit(pmod, *bad, check=True)


def test_values_beyond_n_comp_are_not_looked_at(pmod):
    """A NaN in a component that does not exist (column >= n_comp of V, eigenvalue >= n_comp) flags nothing."""
    V, E, nc, XTY, CW = (t.copy() for t in pc.stopping_rank_case())
    coef, icpt, _, n_fit, info = device_fit(pmod, V, E, nc, XTY, CW)
    V[1, :, 12], E[1, 13] = np.nan, np.nan
    coef_b, icpt_b, _, n_fit_b, info_b = device_fit(pmod, V, E, nc, XTY, CW)
    assert np.array_equal(coef_b, coef) and np.array_equal(icpt_b, icpt) and info_b.tolist() == [1, 1, 1]


def raw_fit(V, E, nc, XTY, CW, ws_bytes, **kw):
    """cvm_pcalda_fit through the C ABI with a workspace of exactly ``ws_bytes``; (rc, coef, intercept, n_fit, info)."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, A = V.shape
    C = XTY.shape[2]
    d = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (V, E, nc, XTY, CW)]
    coef = torch.empty((F, A, K, C), dtype=torch.float64, device="cuda")
    icpt = torch.empty((F, A, C), dtype=torch.float64, device="cuda")
    n_fit = torch.empty((F,), dtype=torch.int32, device="cuda")
    info = torch.empty((F,), dtype=torch.int32, device="cuda")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    args = dict(F=F, K=K, C=C, A=A, dtype=_lib.CVM_F64, tol=0.0)
    args.update(kw)
    rc = lib.cvm_pcalda_fit(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), args["F"],
                            args["K"], args["C"], args["A"], args["dtype"], args["tol"], coef.data_ptr(), icpt.data_ptr(),
                            n_fit.data_ptr(), info.data_ptr(), ws.data_ptr(), ws_bytes,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, coef.cpu().numpy(), icpt.cpu().numpy(), n_fit.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("K,C,A", [(33, 3, 33), (129, 17, 5)])
def test_a_folds_bits_are_its_own(pmod, K, C, A):
    """Two runs give the same bits; fold 1 of a batch of 3 has the bits of the same fold run alone; a workspace of
    two folds and the smallest workspace there is (one fold's record) give the bits of the full workspace; one byte
    less is CVM_EWORKSPACE."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    case = pc.grid_case(K, C, A)
    coef, icpt, _, n_fit, info = device_fit(pmod, *case)
    again = device_fit(pmod, *case)
    assert np.array_equal(again[0], coef) and np.array_equal(again[1], icpt)
    alone = device_fit(pmod, *(t[1:2] for t in case))
    assert np.array_equal(alone[0][0], coef[1]) and np.array_equal(alone[1][0], icpt[1]) and alone[3][0] == n_fit[1]
    one, two, full = (lib.cvm_pcalda_workspace_bytes(n, K, C, A) for n in (1, 2, 3))
    assert 0 < one <= two <= full
    for ws_bytes in (full, two, one):
        rc, c2, i2, n2, f2 = raw_fit(*case, ws_bytes)
        assert rc == _lib.CVM_OK, lib.cvm_last_error()
        assert np.array_equal(c2, coef) and np.array_equal(i2, icpt) and np.array_equal(n2, n_fit) and np.array_equal(f2, info)
    assert raw_fit(*case, one - 1)[0] == _lib.CVM_EWORKSPACE


def test_bad_arguments_through_the_c_abi(pmod):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    case = pc.grid_case(33, 3, 33)
    ws = lib.cvm_pcalda_workspace_bytes(3, 33, 3, 33)
    for kw in (dict(K=0), dict(K=4097), dict(C=1), dict(C=65), dict(A=0), dict(A=34), dict(dtype=5), dict(tol=1.0),
               dict(tol=float("nan")), dict(F=-1)):
        assert raw_fit(*case, ws, **kw)[0] == _lib.CVM_EINVAL, kw
    assert lib.cvm_pcalda_workspace_bytes(3, 100, 3, 65) == 0


def test_no_fold_and_one_matrix(pmod):
    V, E, nc, XTY, CW = pc.grid_case(2, 3, 2)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()          # noqa: E731
    fit = pmod.pcalda_from_components(up(V[:0]), up(E[:0]), up(nc[:0]), up(XTY[:0]), up(CW[:0]))
    assert fit.coef.shape == (0, 2, 2, 3) and fit.intercept.shape == (0, 2, 3) and fit.info.shape == (0,)
    assert fit.n_fit.shape == (0,) and fit.priors.shape == (0, 3)
    coef, icpt, _, n_fit, info = device_fit(pmod, V, E, nc, XTY, CW)
    one = pmod.pcalda_from_components(up(V[0]), up(E[0]), up(nc[0]), up(XTY[0]), up(CW[0]))
    assert one.coef.shape == (1, 2, 2, 3) and np.array_equal(one.coef.cpu().numpy()[0], coef[0])
    assert np.array_equal(one.intercept.cpu().numpy()[0], icpt[0])
    # a single (K, K) / (K, C) pair through the eigensolver: the batch's fold 0 to the bit
    X, y, w = lc.grid_rows(33, 3)
    XTX, XTYm, CWm = lc.batch_inputs(X, y, w, lc.folds_of(X.shape[0], 3), 3)
    batch = pmod.pcalda_fit_batched(up(XTX), up(XTYm), up(CWm), 5)
    single = pmod.pcalda_fit_batched(up(XTX[0]), up(XTYm[0]), up(CWm[0]), 5)
    assert single.coef.shape == (1, 5, 33, 3) and torch.equal(single.coef[0], batch.coef[0])
    assert torch.equal(single.intercept[0], batch.intercept[0]) and torch.equal(single.eigenvalues[0], batch.eigenvalues[0])
    empty = pmod.pcalda_fit_batched(up(XTX[:0]), up(XTYm[:0]), up(CWm[:0]), 5)
    assert empty.coef.shape == (0, 5, 33, 3) and empty.eigenvalues.shape == (0, 5)


@pytest.mark.parametrize("solver", ["scalar", "blocked"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale_X", [False, True])
def test_end_to_end(pmod, weighted, scale_X, solver):
    """CVMatrix.fit -> cv_pcalda -> lda_cv_predict: the labels are the row-based reference's (PCA by the SVD of the
    standardised training rows, lsqr LDA on the scores) on every row whose reference margin exceeds the error
    allowed on a score (no row of the reference falls under it, tests/test_pcalda_host.py; the cap is 1 %);
    lda_cv_decision is cv_predict plus the gathered intercept to the bit; rows in no fold are labelled -1."""
    import cvmatrix_amd as amd
    from cvmatrix_amd import lda
    from cvmatrix_amd.predict import cv_predict
    X, y, w, folds, outside = pc.e2e_rows(weighted)
    C, A = pc.E2E["C"], pc.E2E["A"]
    cvm = amd.CVMatrix(True, False, scale_X, False, dtype=np.float64)
    cvm.fit(X, lc.indicator(y, C), w)
    batch = cvm.prepare_folds(folds)
    fit, stats = pmod.cv_pcalda(cvm, batch, A, solver=solver)
    assert not fit.info.cpu().numpy().any() and np.all(fit.n_fit.cpu().numpy() == A)
    assert fit.coef.shape == (len(folds), A, pc.E2E["K"], C) and fit.eigenvalues.shape == (len(folds), A)
    got = lda.lda_cv_predict(cvm, batch, stats, fit).cpu().numpy()
    scores, allowed, _ = pc.e2e_reference(X, y, w, folds, C, A, scale_X)
    want, decided = pc.decided_rows(scores, allowed)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.all(got[outside] == -1) and np.all(got[np.concatenate(folds)] >= 0)
    inside = np.setdiff1d(np.arange(X.shape[0]), outside)
    skipped = 1.0 - decided[inside].mean(axis=0)
    print("skipped share per number of components:", skipped)
    assert np.all(skipped <= pc.E2E_SKIP_CAP)
    assert np.array_equal(got[decided], want[decided])
    # the decision: cv_predict plus the intercept of the row's fold, to the bit
    dec = lda.lda_cv_decision(cvm, batch, stats, fit).cpu().numpy()
    plain = cv_predict(cvm, batch, (stats[0], stats[1], None, None), fit.coef).cpu().numpy()
    icpt = fit.intercept.cpu().numpy()
    assert np.all(np.isnan(dec[outside]))
    for f, val in enumerate(folds):
        assert np.array_equal(dec[val], plain[val] + icpt[f][None]), f


def test_the_example_agrees_with_sklearn(pmod, monkeypatch):
    """examples/fast_cv_pcalda.py at N = 600, K = 12, C = 3, four folds, 6 components: it asserts its own agreement
    with scikit-learn Pipeline(PCA, LDA(lsqr)) refits per fold."""
    import importlib.util
    import os
    pytest.importorskip("sklearn.discriminant_analysis")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fast_cv_pcalda", os.path.join(root, "examples", "fast_cv_pcalda.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr("sys.argv", ["fast_cv_pcalda.py", "600", "12", "3", "4", "6"])
    acc = mod.main()
    assert acc.shape == (6,) and np.all(acc > 1.0 / 3)
