"""CPU: the host half of the device PCA-LDA -- the argument rules of cvmatrix_amd/pcalda.py before any library
call, the workspace sizing and the argument errors of the C ABI -- and the conditions the GPU tests
(tests/test_gpu_pcalda.py) rest on: the reference of tests/pcalda_cases.py against scikit-learn's
Pipeline(PCA, LinearDiscriminantAnalysis(lsqr)) on the grid's designs, the pivot margins that make an exact
comparison of the stopping decisions fair, the eigenvalue ratios of the end-to-end design and that its reference
leaves out no row at the score-error bound the gate implies."""

import ctypes

import numpy as np
import pytest
import torch

import lda_cases as lc
import pcalda_cases as pc
from cvmatrix_amd import _lib
from cvmatrix_amd import lda, pcalda


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def host(K=8, C=3, F=2, dtype=torch.float64):
    return (torch.eye(K, dtype=dtype).repeat(F, 1, 1), torch.ones((F, K, C), dtype=dtype),
            torch.ones((F, C), dtype=torch.float64))


# ---- the argument rules, without a device

@pytest.mark.parametrize("bad", [0, -1, 65, 2.0, "3", None, True, np.float64(2)])
def test_components_are_refused(bad):
    XTX, XTY, W = host(K=70)
    with pytest.raises(ValueError, match="A must be"):
        pcalda.pcalda_fit_batched(XTX, XTY, W, bad)
    with pytest.raises(ValueError, match="A must be"):
        pcalda.check_components(bad)


def test_components_above_K_are_refused():
    XTX, XTY, W = host(K=8)
    with pytest.raises(ValueError, match="A must be"):
        pcalda.pcalda_fit_batched(XTX, XTY, W, 9)
    assert pcalda.check_components(8, 8) == 8 and pcalda.check_components(np.int64(64), 100) == 64
    assert pcalda.check_components(64) == 64


@pytest.mark.parametrize("bad", [np.nan, 1.0, 1.5, np.inf])
def test_pivot_tol_is_refused(bad):
    XTX, XTY, W = host()
    with pytest.raises(ValueError, match="pivot_tol"):
        pcalda.pcalda_fit_batched(XTX, XTY, W, 2, pivot_tol=bad)
    with pytest.raises(ValueError, match="pivot_tol"):
        pcalda.pcalda_from_components(XTX[:, :, :2], torch.ones((2, 2), dtype=torch.float64),
                                      torch.ones(2, dtype=torch.int32), XTY, W, pivot_tol=bad)
    assert pcalda.check_pivot_tol(None) == 0.0 and pcalda.check_pivot_tol(-1.0) == 0.0
    assert pcalda.check_pivot_tol(1e-6) == 1e-6 and pcalda.DEFAULT_PIVOT_TOL == 2.0 ** -26


@pytest.mark.parametrize("C", [1, 65])
def test_class_counts_are_refused(C):
    XTX, XTY, W = host(C=C)
    with pytest.raises(ValueError, match="classes"):
        pcalda.pcalda_fit_batched(XTX, XTY, W, 2)
    with pytest.raises(ValueError, match="classes"):
        pcalda.pcalda_from_components(XTX[:, :, :2], torch.ones((2, 2), dtype=torch.float64),
                                      torch.ones(2, dtype=torch.int32), XTY, W)


def test_K_above_the_solvers_limit_is_refused():
    XTY, W = torch.ones((1, 513, 2), dtype=torch.float32), torch.ones((1, 2), dtype=torch.float64)
    XTX = torch.zeros((1, 513, 513), dtype=torch.float32)
    with pytest.raises(ValueError, match="blocked"):
        pcalda.pcalda_fit_batched(XTX, XTY, W, 2)
    with pytest.raises(TypeError):                                  # the blocked solver takes it: refused as a host tensor
        pcalda.pcalda_fit_batched(XTX, XTY, W, 2, solver="blocked")
    big = torch.zeros((1, 4097, 4097), dtype=torch.float32)
    with pytest.raises(ValueError, match="4096"):
        pcalda.pcalda_fit_batched(big, torch.ones((1, 4097, 2), dtype=torch.float32), W, 2, solver="blocked")
    with pytest.raises(ValueError, match="solver"):
        pcalda.pcalda_fit_batched(*host(), 2, solver="lapack")


def test_class_weights_are_refused():
    XTX, XTY, W = host(K=8, C=3, F=2)
    for bad in (torch.ones((3, 2), dtype=torch.float64), W.float(), torch.ones(3, dtype=torch.float64),
                torch.ones((2, 3, 1), dtype=torch.float64), torch.ones((2, 3), dtype=torch.int64)):
        with pytest.raises(ValueError, match="class_weights"):
            pcalda.pcalda_fit_batched(XTX, XTY, bad, 2)
        with pytest.raises(ValueError, match="class_weights"):
            pcalda.pcalda_from_components(XTX[:, :, :2], torch.ones((2, 2), dtype=torch.float64),
                                          torch.ones(2, dtype=torch.int32), XTY, bad)
    with pytest.raises(TypeError):
        pcalda.pcalda_fit_batched(XTX, XTY, np.ones((2, 3)), 2)
    with pytest.raises(ValueError, match="one device"):
        lda.check_class_weights(W, 2, 3, torch.device("cuda", 0))   # (a device's name: nothing is touched)


def test_components_eigenvalues_and_counts_are_refused():
    XTX, XTY, W = host(K=8, C=3, F=2)
    V, E, n = XTX[:, :, :4].contiguous(), torch.ones((2, 4), dtype=torch.float64), torch.ones(2, dtype=torch.int32)
    for kw in (dict(eigenvalues=E.float()), dict(eigenvalues=E[:, :3]), dict(n_comp=n.long()), dict(n_comp=n[:1]),
               dict(components=V.float()), dict(components=V[:, :7]), dict(components=V[0])):
        args = dict(components=V, eigenvalues=E, n_comp=n, XTY=XTY, class_weights=W)
        args.update(kw)
        with pytest.raises(ValueError):
            pcalda.pcalda_from_components(**args)
    with pytest.raises(ValueError, match="A must be"):              # A = 65 > 64
        pcalda.pcalda_from_components(torch.ones((1, 70, 65), dtype=torch.float64), torch.ones((1, 65), dtype=torch.float64),
                                      n[:1], torch.ones((1, 70, 3), dtype=torch.float64), W[:1])


def test_host_tensors_and_arrays_are_refused_before_the_device():
    XTX, XTY, W = host()
    with pytest.raises(TypeError):
        pcalda.pcalda_fit_batched(XTX, XTY, W, 2)
    with pytest.raises(TypeError):
        pcalda.pcalda_fit_batched(XTX.numpy(), XTY.numpy(), W.numpy(), 2)
    with pytest.raises(TypeError):
        pcalda.pcalda_from_components(XTX[:, :, :2].contiguous(), torch.ones((2, 2), dtype=torch.float64),
                                      torch.ones(2, dtype=torch.int32), XTY, W)
    with pytest.raises(TypeError):
        pcalda.pcalda_from_components(XTX.numpy()[:, :, :2], np.ones((2, 2)), np.ones(2, dtype=np.int32), XTY.numpy(),
                                      W.numpy())


class _Model:
    """What cv_pcalda looks at before it touches anything else."""
    def __init__(self, center_X, scale_Y):
        self.center_X, self.scale_Y = center_X, scale_Y

    def prepare_folds(self, folds):
        raise AssertionError("cv_pcalda went on with arguments it must refuse")


@pytest.mark.parametrize("center_X,scale_Y", [(False, False), (True, True), (False, True)])
def test_cv_pcalda_refuses_the_model(center_X, scale_Y):
    with pytest.raises(ValueError, match="center_X|scale_Y"):
        pcalda.cv_pcalda(_Model(center_X, scale_Y), [np.arange(3)], 2)


def test_cv_pcalda_refuses_its_arguments_first():
    with pytest.raises(ValueError, match="A must be"):
        pcalda.cv_pcalda(_Model(True, False), [np.arange(3)], 65)
    with pytest.raises(ValueError, match="pivot_tol"):
        pcalda.cv_pcalda(_Model(True, False), [np.arange(3)], 2, pivot_tol=1.0)


def test_the_fit_is_what_lda_cv_decision_takes():
    """lda_cv_decision and lda_cv_predict use ``fit.coef`` and ``fit.intercept`` and nothing else of the fit."""
    assert pcalda.PCALDAFit._fields == ("coef", "intercept", "priors", "n_fit", "info", "eigenvalues")
    assert set(lda.LDAFit._fields) <= set(pcalda.PCALDAFit._fields)
    for fn in (lda.lda_cv_decision, lda.lda_cv_predict):
        # (the names the compiled function looks up as attributes or globals: the docstring is not among them)
        used = set(fn.__code__.co_names) & set(lda.LDAFit._fields + pcalda.PCALDAFit._fields)
        assert used <= {"coef", "intercept"}, used
    assert {"coef", "intercept"} <= set(lda.lda_cv_decision.__code__.co_names)
    fit = pcalda.PCALDAFit(*(torch.zeros(1) for _ in range(6)))
    assert fit.coef is fit[0] and fit.intercept is fit[1]
    assert (pcalda.MAX_K, pcalda.MAX_COMPONENTS, pcalda.WORKSPACE_LIMIT) == (4096, 64, 4 << 30)


# ---- the C ABI, without a device

def test_workspace_bytes_is_host_arithmetic(lib):
    ws = lib.cvm_pcalda_workspace_bytes
    for K, C, A in ((1, 2, 1), (33, 3, 33), (512, 16, 20), (4096, 64, 64)):
        last = 0
        for F in (1, 2, 3, 10, 100, 1000):
            now = ws(F, K, C, A)
            assert now >= last, (K, C, A, F)                       # monotone in F (regions are padded to 256 bytes)
            assert now >= 8 * F * A * (-(-K // pc.KSLICE) * C + A + C)
            last = now
        assert ws(1000, K, C, A) > ws(1, K, C, A)
    assert ws(0, 8, 2, 1) == ws(1, 8, 2, 1)
    for bad in ((1, 0, 2, 1), (1, 4097, 2, 1), (1, 8, 1, 1), (1, 8, 65, 1), (1, 8, 2, 0), (1, 8, 2, 9), (1, 100, 2, 65),
                (-1, 8, 2, 1)):
        assert ws(*bad) == 0, bad


def test_argument_errors_are_decided_before_the_device(lib):
    """K = 0 and 4097, C = 1 and 65, A = 0, above K and above 64, a pivot_tol of 1 and NaN, a dtype that is none, a
    null pointer with F > 0: CVM_EINVAL from arguments alone (the pointers are never followed); n_folds == 0
    launches nothing; less than one fold's record is CVM_EWORKSPACE."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(K=8, C=2, A=2, tol=0.0, dtype=_lib.CVM_F64, F=0, V=p, ws=p, ws_bytes=1 << 20):
        return lib.cvm_pcalda_fit(V, p, p, p, p, F, K, C, A, dtype, tol, p, p, p, p, ws, ws_bytes, None)

    assert call() == _lib.CVM_OK                                   # no fold: nothing is launched
    assert call(V=None, ws=None, ws_bytes=0) == _lib.CVM_OK
    for kw, text in (({"K": 0}, b"K"), ({"K": 4097}, b"K"), ({"C": 1}, b"C"), ({"C": 65}, b"C"), ({"A": 0}, b"A"),
                     ({"A": 9}, b"A"), ({"K": 100, "A": 65}, b"A"), ({"tol": 1.0}, b"pivot_tol"),
                     ({"tol": float("nan")}, b"pivot_tol"), ({"dtype": 7}, b"dtype"), ({"F": -1}, b"shape"),
                     ({"F": 1, "V": None}, b"null"), ({"F": 1, "ws": None}, b"null")):
        assert call(**kw) == _lib.CVM_EINVAL, kw
        assert text in lib.cvm_last_error(), (kw, lib.cvm_last_error())
    one = lib.cvm_pcalda_workspace_bytes(1, 33, 3, 5)
    assert call(K=33, C=3, A=5, F=1, ws_bytes=one - 1) == _lib.CVM_EWORKSPACE
    assert b"workspace" in lib.cvm_last_error()


# ---- the reference is scikit-learn's pipeline

def against_sklearn(X, y, w, folds, C, A, scale=False):
    """(the largest difference of the decision values, each row's less their mean over the classes, relative to the
    largest of them; whether all labels agree): tests/pcalda_cases.truth_fold on the fold's matrices against
    Pipeline(PCA(a + 1, svd_solver="full"), LinearDiscriminantAnalysis(solver="lsqr")) refitted on the fold's
    training rows (replicated by their integer weights), on the fold's validation rows."""
    da = pytest.importorskip("sklearn.discriminant_analysis")
    from sklearn.decomposition import PCA
    from sklearn.pipeline import make_pipeline
    V, E, nc, XTY, CW = pc.batch_inputs(X, y, w, folds, C, A, scale=scale)
    worst, same = 0.0, True
    for f, val in enumerate(folds):
        tr, wt, mu, sd = lc.training_stats(X, w, val, scale)
        coef, icpt = pc.truth_fold(V[f], E[f], XTY[f], CW[f], A)
        Zt, Zv = (X[tr] - mu) / sd, (X[val] - mu) / sd
        rep = np.repeat(np.arange(tr.size), wt.astype(int))
        present = np.flatnonzero(CW[f] > 0)
        for a in range(A):
            sk = make_pipeline(PCA(a + 1, svd_solver="full"), da.LinearDiscriminantAnalysis(solver="lsqr"))
            sk.fit(Zt[rep], y[tr][rep])
            mine = (Zv @ coef[a] + icpt[a])[:, present]
            theirs = sk.decision_function(Zv)
            if present.size == 2:                                   # (scikit-learn's binary form: one column)
                mine, theirs = mine[:, 1] - mine[:, 0], theirs
                same &= bool(np.array_equal(mine > 0, theirs > 0))
            else:
                same &= bool(np.array_equal(present[mine.argmax(axis=1)], sk.predict(Zv)))
                mine, theirs = mine - mine.mean(axis=1, keepdims=True), theirs - theirs.mean(axis=1, keepdims=True)
            worst = max(worst, float(np.abs(mine - theirs).max() / np.abs(theirs).max()))
    return worst, same


SK_GRID = [(K, C, min(A, 8)) for K, C, A in pc.GRID if K <= 65]


@pytest.mark.parametrize("K,C,A", SK_GRID)
def test_reference_is_sklearn_on_the_grid(K, C, A):
    X, y, w = lc.grid_rows(K, C)
    worst, same = against_sklearn(X, y, w, lc.folds_of(X.shape[0], C), C, A)
    assert worst <= 1e-10 and same, worst


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_reference_is_sklearn_end_to_end(weighted, scale):
    X, y, w, folds, _ = pc.e2e_rows(weighted)
    worst, same = against_sklearn(X, y, w, folds, pc.E2E["C"], pc.E2E["A"], scale)
    assert worst <= 1e-10 and same, worst


def test_row_reference_is_the_matrix_reference():
    """The row-based reference of the end-to-end test (SVD of the rows) gives the scores of the matrix-based truth."""
    X, y, w, folds, _ = pc.e2e_rows(True)
    C, A = pc.E2E["C"], pc.E2E["A"]
    V, E, nc, XTY, CW = pc.batch_inputs(X, y, w, folds, C, A, scale=True)
    for f, val in enumerate(folds):
        coef, icpt, _, (mu, sd) = pc.row_reference_fold(X, y, w, val, C, A, True)
        tc, ti = pc.truth_fold(V[f], E[f], XTY[f], CW[f], A)
        Z = (X[val] - mu) / sd
        for a in range(A):
            mine, theirs = Z @ coef[a] + icpt[a], Z @ tc[a] + ti[a]
            mine, theirs = mine - mine.mean(axis=1, keepdims=True), theirs - theirs.mean(axis=1, keepdims=True)
            assert np.abs(mine - theirs).max() <= 1e-9 * np.abs(theirs).max(), (f, a)


# ---- every design meets its own conditions

def test_the_grid_holds_every_size():
    assert {k for k, _, _ in pc.GRID} == set(pc.K_VALUES) and {c for _, c, _ in pc.GRID} == set(pc.C_VALUES)
    assert set(pc.GRID_F32) <= set(pc.GRID) and len(pc.GRID_F32) == 6
    assert pc.KSLICE + 1 in pc.K_VALUES
    for K in pc.K_VALUES:
        assert {a for k, _, a in pc.GRID if k == K} <= {1, 2, min(K, 5), min(K, 64)}
    assert {a for _, _, a in pc.GRID} >= {1, 2, 5, 64}


def all_margins(V, E, nc, XTY, CW):
    return [pc.pivot_margins(V[f], E[f], nc[f], XTY[f], CW[f]) for f in range(V.shape[0])]


@pytest.mark.parametrize("K,C,A", pc.GRID)
def test_pivot_margins_on_the_grid(K, C, A):
    """Every pivot of every grid design is accepted with a margin of 100 and more: all A models exist."""
    V, E, nc, XTY, CW = pc.grid_case(K, C, A)
    assert np.all(nc == A)
    for f in range(pc.N_FOLDS):
        assert pc.reference_path(V[f], E[f], nc[f], XTY[f], CW[f])[:2] == (A, 0)
    assert min(m[0] for m in all_margins(V, E, nc, XTY, CW)) >= 100.0


def test_pivot_margins_on_the_ladder_and_the_absent_class():
    """The ladder runs with pivot_tol = 2^-40: at 1e4 standard deviations between the classes the within-class share
    of the leading components is 1e-8, which is where the default threshold sits on purpose."""
    cases = [(pc.ladder_case(sep), pc.LADDER_PIVOT_TOL) for sep in pc.LADDER_SEP] + [(pc.absent_case(), pc.PIVOT_TOL)]
    for case, tol in cases:
        V, E, nc, XTY, CW = case
        for f in range(V.shape[0]):
            assert pc.reference_path(V[f], E[f], nc[f], XTY[f], CW[f], tol)[:2] == (V.shape[2], 0)
            assert pc.pivot_margins(V[f], E[f], nc[f], XTY[f], CW[f], tol)[0] >= 100.0
    V, E, nc, XTY, CW = pc.ladder_case(pc.LADDER_SEP[-1])
    assert min(pc.pivot_margins(V[f], E[f], nc[f], XTY[f], CW[f])[0] for f in range(3)) < 100.0      # (the default would not do)
    assert pc.absent_case()[4][1, 2] == 0.0


def test_the_stopping_designs_stop_where_they_are_wanted():
    V, E, nc, XTY, CW = pc.stopping_pivot_case()
    paths = [pc.reference_path(V[f], E[f], nc[f], XTY[f], CW[f])[:2] for f in range(3)]
    assert paths == [(32, 0), (27, 2), (32, 0)] and nc[1] >= 28
    margins = all_margins(V, E, nc, XTY, CW)
    print("K = 40 on 30 rows: accepted / rejected margins", margins[1])
    assert all(m[0] >= 100.0 for m in margins) and margins[1][1] <= 0.01

    V, E, nc, XTY, CW = pc.stopping_rank_case()
    assert nc.tolist() == [10, 10, 10] and V.shape[2] == 16
    assert [pc.reference_path(V[f], E[f], nc[f], XTY[f], CW[f])[:2] for f in range(3)] == [(10, 1)] * 3
    assert min(m[0] for m in all_margins(V, E, nc, XTY, CW)) >= 100.0

    V, E, nc, XTY, CW = pc.separated_case()
    paths = [pc.reference_path(V[f], E[f], nc[f], XTY[f], CW[f])[:2] for f in range(3)]
    assert paths == [(4, 0), (0, 2), (4, 0)] and nc.tolist() == [4, 4, 4]
    margins = all_margins(V, E, nc, XTY, CW)
    print("separated classes: rejected margin", margins[1][1])
    assert margins[1][1] <= 0.01 and margins[0][0] >= 100.0 and margins[2][0] >= 100.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("scale", [False, True])
def test_the_end_to_end_design(weighted, scale):
    """Consecutive eigenvalue ratios of 1.1 and more for every a <= A on every fold; every pivot accepted with
    margin; and the reference leaves out NO row at the score-error bound the gate implies.  Rows in no fold exist
    and are labelled -1; the classes are learnable."""
    X, y, w, folds, outside = pc.e2e_rows(weighted)
    C, A = pc.E2E["C"], pc.E2E["A"]
    scores, allowed, ratios = pc.e2e_reference(X, y, w, folds, C, A, scale)
    print("smallest eigenvalue ratio", ratios.min(), "largest allowed error", np.nanmax(allowed, axis=0))
    assert ratios.shape == (pc.E2E["F"], A) and ratios.min() >= 1.1
    case = pc.batch_inputs(X, y, w, folds, C, A, scale=scale)
    assert min(m[0] for m in all_margins(*case)) >= 100.0 and np.all(case[2] == A)
    labels, decided = pc.decided_rows(scores, allowed)
    inside = np.setdiff1d(np.arange(X.shape[0]), outside)
    assert outside.size >= 50 and np.all(labels[outside] == -1) and not decided[outside].any()
    assert decided[inside].all()
    acc = (labels[inside] == y[inside, None]).mean(axis=0)
    print("accuracy per number of components", acc)
    assert np.all(acc > 0.4) and acc[-1] > 0.6
