"""GPU (-m gpu): the device LDA (cvm_lda_fit through cvmatrix_amd/lda.py) against the reference and the gate of
tests/lda_cases.py -- err <= 2 Y + c u (float32: + 2^-24), derived there and not calibrated -- and the rules of
include/cvmhip.h: a fold's bits depend on its own inputs alone, absent classes, singular scatters, flagged folds.
The inputs of the accuracy tests are formed by NumPy in float64 and uploaded, so that the device and the
yardstick see the same bits.

Where the kernels land on the MI355X (CVM_LDA_REPORT), the largest err / Y per test: DESIGN.md 4.15."""

import functools

import numpy as np
import pytest
import torch

import lda_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lmod(hip_device):
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import lda as mod
    return mod


def device_fit(lmod, XTX, XTY, CW, gammas=lc.GAMMAS, **kw):
    """lda_fit_batched on uploaded copies; (coef, intercept, priors, info) as NumPy arrays."""
    fit = lmod.lda_fit_batched(torch.from_numpy(XTX).cuda(), torch.from_numpy(XTY).cuda(),
                               torch.from_numpy(CW).cuda(), gammas, **kw)
    return tuple(t.cpu().numpy() for t in fit)


@functools.lru_cache(maxsize=None)
def grid_case(K, C):
    X, y, w = lc.grid_rows(K, C)
    folds = lc.folds_of(X.shape[0], C)
    return lc.batch_inputs(X, y, w, folds, C), lc.reference_batch(X, y, w, folds, C)


@pytest.mark.parametrize("K,C,dtype", [(K, C, np.float64) for K, C in lc.GRID] +
                         [(K, C, np.float32) for K, C in lc.GRID_F32])
def test_shape_grid(lmod, K, C, dtype):
    (XTX, XTY, CW), refs = grid_case(K, C)
    XTX, XTY = XTX.astype(dtype), XTY.astype(dtype)
    coef, icpt, priors, info = device_fit(lmod, XTX, XTY, CW)
    assert coef.shape == (3, 4, K, C) and icpt.shape == (3, 4, C) and coef.dtype == dtype and icpt.dtype == dtype
    assert info.shape == (3, 4) and info.dtype == np.int32 and not info.any()
    assert priors.dtype == np.float64 and np.array_equal(priors, CW / CW.sum(axis=1, keepdims=True))
    worst = lc.assert_gate(coef, icpt, XTX, XTY, CW, refs, f"grid K={K} C={C} {np.dtype(dtype).name}",
                           float32=dtype == np.float32)
    print(f"K={K} C={C} {np.dtype(dtype).name}: largest err / Y {worst:.3f}")


@pytest.mark.parametrize("sep", lc.LADDER_SEP)
def test_cancellation_ladder(lmod, sep):
    """Class means 1, 1e2 and 1e4 within-class standard deviations apart: XTX is up to 1e7 times S_w and the
    downdate loses that many digits, in the device and in the yardstick alike."""
    X, y, w = lc.ladder_rows(sep)
    C = lc.LADDER_KC[1]
    folds = lc.folds_of(X.shape[0], C)
    XTX, XTY, CW = lc.batch_inputs(X, y, w, folds, C)
    refs = lc.reference_batch(X, y, w, folds, C)
    coef, icpt, _, info = device_fit(lmod, XTX, XTY, CW)
    assert not info.any()
    worst = lc.assert_gate(coef, icpt, XTX, XTY, CW, refs, f"ladder sep={sep:g}")
    print(f"sep={sep:g}: kappa {lc.kappa(XTX, refs[3]):.3g}, largest err / Y {worst:.3f}")


def raw_fit(XTX, XTY, CW, gammas, ws_bytes):
    """cvm_lda_fit through the C ABI with a workspace of exactly ``ws_bytes``."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, C = XTY.shape
    L = len(gammas)
    dX, dY, dW = (torch.from_numpy(a).cuda() for a in (XTX, XTY, CW))
    coef = torch.empty((F, L, K, C), dtype=torch.float64, device="cuda")
    icpt = torch.empty((F, L, C), dtype=torch.float64, device="cuda")
    info = torch.empty((F, L), dtype=torch.int32, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    g = np.ascontiguousarray(gammas, dtype=np.float64)
    rc = lib.cvm_lda_fit(dX.data_ptr(), dY.data_ptr(), dW.data_ptr(), F, K, C, g.ctypes.data, L, _lib.CVM_F64,
                         coef.data_ptr(), icpt.data_ptr(), info.data_ptr(), ws.data_ptr(), ws_bytes,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.CVM_OK, lib.cvm_last_error()
    torch.cuda.synchronize()
    return coef.cpu().numpy(), icpt.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("K,C", [(33, 3), (64, 17)])
def test_a_folds_bits_are_its_own(lmod, K, C):
    """Fold 1 of a batch of 3 has the bits of the same fold run alone; a workspace of exactly one fold, and the
    smallest workspace there is (one fold record, one factorisation), give the bits of the full workspace."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    (XTX, XTY, CW), _ = grid_case(K, C)
    coef, icpt, _, info = device_fit(lmod, XTX, XTY, CW)
    coef1, icpt1, _, info1 = device_fit(lmod, XTX[1:2], XTY[1:2], CW[1:2])
    assert np.array_equal(coef[1], coef1[0]) and np.array_equal(icpt[1], icpt1[0]) and np.array_equal(info[1], info1[0])
    L = len(lc.GAMMAS)
    one_fold = lib.cvm_lda_workspace_bytes(1, K, C, L)
    smallest = one_fold - lib.cvm_ridge_workspace_bytes(1, K, C, L) + lib.cvm_ridge_workspace_bytes(1, K, C, 1)
    assert smallest < one_fold < lib.cvm_lda_workspace_bytes(3, K, C, L)
    for ws_bytes in (one_fold, smallest):
        c2, i2, f2 = raw_fit(XTX, XTY, CW, lc.GAMMAS, ws_bytes)
        assert np.array_equal(c2, coef) and np.array_equal(i2, icpt) and np.array_equal(f2, info), ws_bytes


def test_absent_class(lmod):
    """Fold 1 trains without class 2: coef 0, intercept -inf and priors 0 for that class there; the other classes
    pass the gate against a reference fitted on the present classes; the other folds have the bits they have
    when run without fold 1."""
    X, y, folds, C = lc.absent_case()
    XTX, XTY, CW = lc.batch_inputs(X, y, None, folds, C)
    refs = lc.reference_batch(X, y, None, folds, C)
    coef, icpt, priors, info = device_fit(lmod, XTX, XTY, CW)
    assert not info.any()
    assert not coef[1, :, :, 2].any() and np.all(np.isneginf(icpt[1, :, 2])) and priors[1, 2] == 0.0
    assert np.all(np.isfinite(np.delete(icpt, 2, axis=2))) and np.all(np.isfinite(icpt[[0, 2]]))
    assert np.all(np.isfinite(coef)) and np.all(priors[[0, 2]] > 0)
    worst = lc.assert_gate(coef, icpt, XTX, XTY, CW, refs, "absent class")
    print(f"absent class: largest err / Y {worst:.3f}")
    others = device_fit(lmod, XTX[[0, 2]], XTY[[0, 2]], CW[[0, 2]])
    assert np.array_equal(others[0], coef[[0, 2]]) and np.array_equal(others[1], icpt[[0, 2]])


def test_singular_scatter(lmod):
    """K = 40 with 30 training rows in fold 1: info > 0 and NaN at g = 0 there, and only there; the same fold at
    g = 0.1, 0.5 and 1 is finite and within the gate, as are the other folds."""
    X, y, folds, C = lc.singular_case()
    XTX, XTY, CW = lc.batch_inputs(X, y, None, folds, C)
    coef, icpt, _, info = device_fit(lmod, XTX, XTY, CW)
    assert 0 < info[1, 0] <= 40 and not info[1, 1:].any() and not info[[0, 2]].any()
    assert np.all(np.isnan(coef[1, 0])) and np.all(np.isnan(icpt[1, 0]))
    assert np.all(np.isfinite(coef[1, 1:])) and np.all(np.isfinite(icpt[1, 1:])) and np.all(np.isfinite(coef[[0, 2]]))
    refs = lc.reference_batch(X, y, None, folds, C, lc.GAMMAS[1:])
    worst = lc.assert_gate(coef[:, 1:], icpt[:, 1:], XTX, XTY, CW, refs, "singular", gammas=lc.GAMMAS[1:])
    print(f"singular: largest err / Y {worst:.3f}")
    with pytest.raises(np.linalg.LinAlgError, match=r"fold 1, shrinkage\[0\]"):
        device_fit(lmod, XTX, XTY, CW, check=True)


def poison(kind, XTX, XTY, CW):
    """Fold 1 of copies of the batch made unusable."""
    XTX, XTY, CW = XTX.copy(), XTY.copy(), CW.copy()
    K = XTX.shape[1]
    if kind == "nan in XTX, upper":
        XTX[1, 0, K - 1] = np.nan
    elif kind == "nan in XTX, lower":
        XTX[1, K - 1, 0] = np.nan
    elif kind == "inf in XTY":
        XTY[1, K // 2, 1] = np.inf
    elif kind == "negative class weight":
        CW[1, 0] = -CW[1, 0]
    elif kind == "nan class weight":
        CW[1, 2] = np.nan
    elif kind == "zero trace":
        Z, H, cw = lc.zero_trace_inputs(K, CW.shape[1])
        XTX[1], XTY[1], CW[1] = Z, H, cw
    return XTX, XTY, CW


@pytest.mark.parametrize("kind", ["nan in XTX, upper", "nan in XTX, lower", "inf in XTY", "negative class weight",
                                  "nan class weight", "zero trace"])
def test_flagged_fold(lmod, kind):
    """The flagged fold has info -1 and NaN in every coef and intercept; the other folds keep their bits."""
    K, C = 33, 3
    (XTX, XTY, CW), _ = grid_case(K, C)
    coef, icpt, _, info = device_fit(lmod, XTX, XTY, CW)
    bad = poison(kind, XTX, XTY, CW)
    coef_b, icpt_b, _, info_b = device_fit(lmod, *bad)
    assert np.all(info_b[1] == -1) and not info_b[[0, 2]].any()
    assert np.all(np.isnan(coef_b[1])) and np.all(np.isnan(icpt_b[1]))
    assert np.array_equal(coef_b[[0, 2]], coef[[0, 2]]) and np.array_equal(icpt_b[[0, 2]], icpt[[0, 2]])
    with pytest.raises(np.linalg.LinAlgError, match="fold 1"):
        device_fit(lmod, *bad, check=True)


def test_no_fold_and_one_matrix(lmod):
    (XTX, XTY, CW), _ = grid_case(2, 2)
    fit = lmod.lda_fit_batched(torch.from_numpy(XTX[:0]).cuda(), torch.from_numpy(XTY[:0]).cuda(),
                               torch.from_numpy(CW[:0]).cuda(), [0.1, 1.0])
    assert fit.coef.shape == (0, 2, 2, 2) and fit.intercept.shape == (0, 2, 2) and fit.info.shape == (0, 2)
    coef, icpt, _, info = device_fit(lmod, XTX, XTY, CW, 0.25)
    one = lmod.lda_fit_batched(torch.from_numpy(XTX[0]).cuda(), torch.from_numpy(XTY[0]).cuda(),
                               torch.from_numpy(CW[0]).cuda(), 0.25)
    assert one.coef.shape == (1, 1, 2, 2) and np.array_equal(one.coef.cpu().numpy()[0], coef[0])
    assert np.array_equal(one.intercept.cpu().numpy()[0], icpt[0])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale_X", [False, True])
def test_end_to_end(lmod, weighted, scale_X):
    """CVMatrix.fit -> training_XTX_XTY_batched -> cv_lda -> lda_cv_predict: the labels are the reference's on
    every row whose reference margin exceeds the error the gate allows on a score (at most 1 % of the rows fall
    under it, tests/test_lda_host.py); lda_cv_decision is cv_predict plus the gathered intercept to the bit; rows
    in no fold are labelled -1."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.predict import cv_predict
    X, y, w, folds, outside = lc.e2e_rows(weighted)
    C = lc.E2E["C"]
    cvm = amd.CVMatrix(True, False, scale_X, False, dtype=np.float64)
    cvm.fit(X, lc.indicator(y, C), w)
    batch = cvm.prepare_folds(folds)
    fit, stats = lmod.cv_lda(cvm, batch, lc.GAMMAS)
    assert not fit.info.cpu().numpy().any()
    XTXr, XTYr, CWr = lc.batch_inputs(X, y, w, folds, C, scale=scale_X)
    assert np.array_equal(lmod.training_class_weights(cvm, batch).cpu().numpy(), CWr)      # sums of small integers
    assert np.array_equal(fit.priors.cpu().numpy(), CWr / CWr.sum(axis=1, keepdims=True))
    got = lmod.lda_cv_predict(cvm, batch, stats, fit).cpu().numpy()
    scores, allowed = lc.reference_scores(X, y, w, folds, C, scale=scale_X)
    want, decided = lc.decided_rows(scores, allowed)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.all(got[outside] == -1) and np.all(got[np.concatenate(folds)] >= 0)
    inside = np.setdiff1d(np.arange(X.shape[0]), outside)
    skipped = 1.0 - decided[inside].mean(axis=0)
    print("skipped share per shrinkage:", skipped)
    assert np.all(skipped <= lc.E2E_SKIP_CAP)
    assert np.array_equal(got[decided], want[decided])
    # the decision: cv_predict plus the intercept of the row's fold, to the bit
    dec = lmod.lda_cv_decision(cvm, batch, stats, fit).cpu().numpy()
    plain = cv_predict(cvm, batch, (stats[0], stats[1], None, None), fit.coef).cpu().numpy()
    icpt = fit.intercept.cpu().numpy()
    assert np.all(np.isnan(dec[outside]))
    for f, val in enumerate(folds):
        assert np.array_equal(dec[val], plain[val] + icpt[f][None]), f
    by_fold = lmod.lda_cv_decision(cvm, batch, stats, fit, order="folds").cpu().numpy()
    assert np.array_equal(by_fold, dec[np.concatenate(folds)])


def test_the_example_agrees_with_sklearn(lmod, monkeypatch):
    """examples/fast_cv_lda.py at N = 600, K = 12, C = 3, four folds: it asserts its own agreement with
    scikit-learn refits (at most one row in 1e4 labelled differently)."""
    import importlib.util
    import os
    pytest.importorskip("sklearn.discriminant_analysis")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fast_cv_lda", os.path.join(root, "examples", "fast_cv_lda.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr("sys.argv", ["fast_cv_lda.py", "600", "12", "3", "4"])
    acc = mod.main()
    assert acc.shape == (8,) and np.all(acc > 1.0 / 3)
