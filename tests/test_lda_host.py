"""CPU: the host half of the device LDA -- the argument rules of cvmatrix_amd/lda.py before any library call, the
workspace sizing and the argument errors of the C ABI -- and the conditions the GPU tests (tests/test_gpu_lda.py)
rest on: the NumPy restatement of tests/lda_cases.py against scikit-learn's lsqr LDA on every design, and that
every design meets its own conditions (the singularity, the absent class, the zero trace, the share of rows the
end-to-end test may skip)."""

import ctypes

import numpy as np
import pytest
import torch

import lda_cases as lc
from cvmatrix_amd import _lib
from cvmatrix_amd import lda


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


A3 = torch.eye(3, dtype=torch.float64)
Y3 = torch.ones((3, 2), dtype=torch.float64)
W3 = torch.ones((1, 2), dtype=torch.float64)


@pytest.mark.parametrize("bad", [-0.1, 1.5, np.nan, [0.0, np.nan], [0.5, 1.0000001], np.inf, [[0.1]], [],
                                 np.linspace(0, 1, 257)])
def test_shrinkage_is_refused(bad):
    with pytest.raises(ValueError):
        lda.check_shrinkage(bad)
    with pytest.raises(ValueError):
        lda.lda_fit_batched(A3, Y3, W3, bad)          # (before the tensors are looked at: they are host tensors)


def test_shrinkage_is_accepted():
    assert lda.check_shrinkage(0.25).tolist() == [0.25] and lda.check_shrinkage(0).dtype == np.float64
    assert lda.check_shrinkage([0, 0.1, 1]).tolist() == [0.0, 0.1, 1.0]
    assert lda.check_shrinkage(np.linspace(0, 1, 256)).size == 256
    assert (lda.MAX_K, lda.MIN_CLASSES, lda.MAX_CLASSES, lda.MAX_SHRINKAGES) == (4096, 2, 64, 256)
    assert lda.LDAFit._fields == ("coef", "intercept", "priors", "info") and lda.WORKSPACE_LIMIT == 4 << 30


@pytest.mark.parametrize("K,C", [(4097, 3), (0, 3), (8, 1), (8, 65), (8, 0)])
def test_shapes_are_refused(K, C):
    with pytest.raises(ValueError):
        lda.check_dims(K, C)


def test_class_weights_are_refused():
    dev = torch.device("cpu")
    ok = torch.ones((3, 4), dtype=torch.float64)
    assert lda.check_class_weights(ok, 3, 4, dev).shape == (3, 4)
    assert lda.check_class_weights(torch.ones(4, dtype=torch.float64), 1, 4, dev).shape == (1, 4)
    for bad in (torch.ones((4, 3), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float32),
                torch.ones(4, dtype=torch.float64), torch.ones((3, 4, 1), dtype=torch.float64),
                torch.ones((3, 4), dtype=torch.int64)):
        with pytest.raises(ValueError):
            lda.check_class_weights(bad, 3, 4, dev)
    with pytest.raises(TypeError):
        lda.check_class_weights(np.ones((3, 4)), 3, 4, dev)
    with pytest.raises(ValueError, match="one device"):
        lda.check_class_weights(ok, 3, 4, torch.device("cuda", 0))        # (a device's name: nothing is touched)


def test_host_tensors_are_refused_before_the_device():
    with pytest.raises(TypeError):
        lda.lda_fit_batched(A3, Y3, W3, 0.1)
    with pytest.raises(TypeError):
        lda.lda_fit_batched(np.eye(3), np.ones((3, 2)), np.ones((1, 2)))


class _Model:
    """What cv_lda looks at before it touches anything else."""
    def __init__(self, center_X, scale_Y):
        self.center_X, self.scale_Y = center_X, scale_Y

    def prepare_folds(self, folds):
        raise AssertionError("cv_lda went on with a model it must refuse")


@pytest.mark.parametrize("center_X,scale_Y", [(False, False), (True, True), (False, True)])
def test_cv_lda_refuses_the_model(center_X, scale_Y):
    with pytest.raises(ValueError):
        lda.cv_lda(_Model(center_X, scale_Y), [np.arange(3)], 0.1)


def test_cv_lda_refuses_the_shrinkage_first():
    with pytest.raises(ValueError, match="shrinkage"):
        lda.cv_lda(_Model(True, False), [np.arange(3)], 1.5)


def test_workspace_bytes_is_host_arithmetic(lib):
    ws, rws = lib.cvm_lda_workspace_bytes, lib.cvm_ridge_workspace_bytes
    for K, C, L in ((1, 2, 1), (33, 3, 4), (512, 16, 20), (4096, 64, 256)):
        last = 0
        for F in (1, 2, 3, 10, 100, 1000):
            now = ws(F, K, C, L)
            assert now > last, (K, C, L, F)                    # monotone in F
            assert now >= rws(F, K, C, L) + 8 * F * K * (K + C + L * C)
            last = now
        one = ws(1, K, C, L) - rws(1, K, C, L) + rws(1, K, C, 1)
        assert 0 < one <= ws(1, K, C, L)
    assert ws(0, 8, 2, 1) == ws(1, 8, 2, 1)
    for bad in ((1, 0, 2, 1), (1, 4097, 2, 1), (1, 8, 1, 1), (1, 8, 65, 1), (1, 8, 2, 0), (1, 8, 2, 257), (-1, 8, 2, 1)):
        assert ws(*bad) == 0, bad


def test_argument_errors_are_decided_before_the_device(lib):
    """K = 0 and 4097, C = 1 and 65, L = 0 and 257, a shrinkage below 0, above 1 and NaN, a dtype that is none, a
    null pointer: CVM_EINVAL from arguments alone (the pointers are never followed); n_folds == 0 launches
    nothing; less than one fold and one factorisation is CVM_EWORKSPACE."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    grid = (ctypes.c_double * 257)(*([0.5] * 257))

    def call(K=8, C=2, L=2, g0=0.5, dtype=_lib.CVM_F64, F=0, XTX=p, ws_bytes=1 << 20):
        grid[0] = g0
        return lib.cvm_lda_fit(XTX, p, p, F, K, C, ctypes.addressof(grid), L, dtype, p, p, p, p, ws_bytes, None)

    assert call() == _lib.CVM_OK                                   # no fold: nothing is launched
    for kw, text in (({"K": 0}, b"K"), ({"K": 4097}, b"K"), ({"C": 1}, b"C"), ({"C": 65}, b"C"), ({"L": 0}, b"L"),
                     ({"L": 257}, b"L"), ({"g0": -1e-9}, b"shrinkage"), ({"g0": 1.0 + 1e-9}, b"shrinkage"),
                     ({"g0": float("nan")}, b"shrinkage"), ({"dtype": 7}, b"dtype"), ({"XTX": None}, b"null"),
                     ({"F": -1}, b"shape")):
        assert call(**kw) == _lib.CVM_EINVAL, kw
        assert text in lib.cvm_last_error(), (kw, lib.cvm_last_error())
    K, C, L = 33, 3, 4
    one = (lib.cvm_lda_workspace_bytes(1, K, C, L) - lib.cvm_ridge_workspace_bytes(1, K, C, L)
           + lib.cvm_ridge_workspace_bytes(1, K, C, 1))
    assert call(K=K, C=C, L=L, ws_bytes=one - 1) == _lib.CVM_EWORKSPACE
    assert call(K=K, C=C, L=L, ws_bytes=one) == _lib.CVM_OK


# ---- the restatement is scikit-learn's lsqr LDA

def log_softmax(s):
    s = s - s.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


def against_sklearn(X, y, w, folds, C, gammas, scale=False, decision=False):
    """The largest difference in predict_log_proba over the folds and the grid: the restatement on the fold's
    training matrices against LinearDiscriminantAnalysis(solver="lsqr", shrinkage=g) refitted on the fold's
    training rows (replicated by their integer weights), on the fold's validation rows.  ``decision``: the
    difference in decision_function instead, each row's scores less their mean over the classes (the term
    common to all classes), relative to the largest of them."""
    da = pytest.importorskip("sklearn.discriminant_analysis")
    worst = 0.0
    for val in folds:
        tr, wt, mu, sd = lc.training_stats(X, w, val, scale)
        XTX, XTY, cw = lc.fold_inputs(X, y, w, val, C, scale)
        coef, icpt = lc.restate(XTX, XTY, cw, gammas)
        Zt, Zv = (X[tr] - mu) / sd, (X[val] - mu) / sd
        rep = np.repeat(np.arange(tr.size), wt.astype(int))
        present = np.flatnonzero(cw > 0)
        for l, g in enumerate(gammas):
            sk = da.LinearDiscriminantAnalysis(solver="lsqr", shrinkage=float(g)).fit(Zt[rep], y[tr][rep])
            assert np.array_equal(sk.classes_, present)
            mine = (Zv @ coef[l] + icpt[l])[:, present]
            if decision:
                theirs = sk.decision_function(Zv)
                mine, theirs = mine - mine.mean(axis=1, keepdims=True), theirs - theirs.mean(axis=1, keepdims=True)
                worst = max(worst, float(np.abs(mine - theirs).max() / np.abs(theirs).max()))
            else:
                worst = max(worst, float(np.abs(log_softmax(mine) - sk.predict_log_proba(Zv)).max()))
    return worst


@pytest.mark.parametrize("K,C", lc.GRID)
def test_restatement_is_sklearn_on_the_grid(K, C):
    X, y, w = lc.grid_rows(K, C)
    assert against_sklearn(X, y, w, lc.folds_of(X.shape[0], C), C, lc.GAMMAS) <= 1e-10


@pytest.mark.parametrize("sep", lc.LADDER_SEP)
def test_restatement_is_sklearn_on_the_ladder(sep):
    """predict_log_proba at one standard deviation between the classes.  Beyond, scikit-learn's is no yardstick:
    it takes the logarithm of probabilities that have underflowed (and lifts the zeros to the smallest normal
    number), so from 1e2 standard deviations on the scores themselves are compared, relative to the largest.
    The bound grows with the cancellation the ladder is there for: the downdate perturbs S_w by
    gate_c(C, kappa) u relative (tests/lda_cases.py), the solve multiplies that by cond(S_w) at most."""
    X, y, w = lc.ladder_rows(sep)
    C = lc.LADDER_KC[1]
    folds = lc.folds_of(X.shape[0], C)
    XTX, _, _ = lc.batch_inputs(X, y, w, folds, C)
    Sw = lc.reference_batch(X, y, w, folds, C)[3]
    bound = 1e-10 + lc.gate_c(C, lc.kappa(XTX, Sw)) * lc.U * max(np.linalg.cond(S) for S in Sw)
    got = against_sklearn(X, y, w, folds, C, lc.GAMMAS, decision=sep > 1.0)
    print(f"sep {sep:g}: kappa {lc.kappa(XTX, Sw):.3g}, difference {got:.3g}, bound {bound:.3g}")
    assert got <= bound


def test_restatement_is_sklearn_on_the_special_designs():
    X, y, folds, C = lc.absent_case()
    assert against_sklearn(X, y, None, folds, C, lc.GAMMAS) <= 1e-10
    X, y, folds, C = lc.singular_case()
    assert against_sklearn(X, y, None, folds, C, lc.GAMMAS[1:]) <= 1e-10     # (g = 0 is singular in fold 1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_restatement_is_sklearn_end_to_end(weighted, scale):
    X, y, w, folds, _ = lc.e2e_rows(weighted)
    assert against_sklearn(X, y, w, folds, lc.E2E["C"], lc.GAMMAS, scale) <= 1e-10


# ---- every design meets its own conditions

def test_the_grid_holds_every_size():
    assert {k for k, _ in lc.GRID} == set(lc.K_VALUES) and {c for _, c in lc.GRID} == set(lc.C_VALUES)
    assert set(lc.GRID_F32) <= set(lc.GRID) and len(lc.GRID_F32) == 6 and 18 <= len(lc.GRID) <= 22
    for K, C in lc.GRID:
        X, y, _ = lc.grid_rows(K, C)
        folds = lc.folds_of(X.shape[0], C)
        _, _, CW = lc.batch_inputs(X, y, None, folds, C)
        assert len(folds) == 3 and np.all(CW >= 2), (K, C)       # every class in every training set, twice
        assert np.all(CW.sum(axis=1) - C >= 4 * K), (K, C)       # rank of S_w with room
        assert len({v.tobytes() for v in folds}) == 3


def test_the_absent_class_is_absent_where_it_is_wanted():
    X, y, folds, C = lc.absent_case()
    _, _, CW = lc.batch_inputs(X, y, None, folds, C)
    assert CW[1, 2] == 0 and np.all(np.delete(CW[1], 2) > 10) and np.all(CW[[0, 2]] > 10)
    coef, icpt, _, _ = lc.reference_fold(X, y, None, folds[1], C)
    assert not coef[:, :, 2].any() and np.all(np.isneginf(icpt[:, 2])) and np.all(np.isfinite(np.delete(icpt, 2, 1)))


def test_the_singular_design_is_singular_where_it_is_wanted():
    X, y, folds, C = lc.singular_case()
    XTX, XTY, CW = lc.batch_inputs(X, y, None, folds, C)
    assert CW.sum(axis=1).tolist() == [140.0, 30.0, 140.0]
    for f in range(3):
        Sw = lc.reference_fold(X, y, None, folds[f], C, lc.GAMMAS[1:])[3]
        ev = np.linalg.eigvalsh(Sw)
        if f == 1:
            assert np.sum(ev > 1e-10 * ev[-1]) == 27                    # 30 rows, 3 class means
        else:
            assert ev[0] > 1e-3 * ev[-1]


def test_the_zero_trace_design_downdates_to_zero():
    XTX, XTY, cw = lc.zero_trace_inputs()
    M = XTY / cw
    assert np.array_equal(M * cw, XTY) and not (XTX - M @ XTY.T).any() and np.array_equal(XTX, XTX.T)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_the_end_to_end_design_skips_few_rows(weighted, scale):
    """The reference alone stays within the cap: at most 1 % of the rows in a fold have a margin at or below the
    error the gate allows on a score.  Rows in no fold exist and are labelled -1."""
    X, y, w, folds, outside = lc.e2e_rows(weighted)
    scores, allowed = lc.reference_scores(X, y, w, folds, lc.E2E["C"], scale=scale)
    labels, decided = lc.decided_rows(scores, allowed)
    inside = np.setdiff1d(np.arange(X.shape[0]), outside)
    assert outside.size >= 50 and np.all(labels[outside] == -1) and not decided[outside].any()
    skipped = 1.0 - decided[inside].mean(axis=0)
    print("skipped share per shrinkage:", skipped, "largest allowed error:", np.nanmax(allowed, axis=0))
    assert np.all(skipped <= lc.E2E_SKIP_CAP)
    acc = (labels[inside] == y[inside, None]).mean(axis=0)
    assert np.all(acc > 0.6)                                        # the classes are learnable: the labels mean something
