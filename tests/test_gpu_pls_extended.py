"""GPU (-m gpu): the device PLS (cvm_pls_fit) where tests/test_gpu_pls.py cannot see it.

Follow-the-weights.  The kernel takes each weight vector from repeated squaring, the oracle from LAPACK, and
the 1e-9 gate of tests/test_gpu_pls.py exists to absorb that difference.  Given the SAME weight vectors
everything else in a component (r, u = XTX r, tTt, p, q, the deflation, B) is determined, so here the
reference is ``ikpls_follow(XTX, XTY, W_kernel)`` in longdouble and the gate per component on B, P, Q, R is

    rel err <= 2 Y + 4 u,      u = 2^-53,

with Y the error of the float64 NumPy restatement against the longdouble one on the same case (three orders
of the variables, the largest; tests/pls_cases.py, tests/test_pls_extended_oracle.py: Y <= 1e-13 for every
component of every case, so none is left out).  No sign fix-ups: the factors follow the kernel's own w.  The
weight vectors are judged on their own: unit norm to 4 u and, for M > 1, a Rayleigh deficit
1 - |Y_a^T w|^2 / lambda_max(Y_a^T Y_a) of at most twice the largest deficit of the oracle's restatement of
the squaring on the same case plus 64 u |XTY|_F / sigma_1(Y_a) -- any dominant vector is right where the
leading singular values are close or equal.

Contract tests: a non-finite fold is NaN throughout with n_fit -1 (include/cvmhip.h), exhaustion is exact,
every output element is written and nothing else, the workspace's content, a fold's place in the batch and
powers of two in the scale of the inputs do not change a bit beyond the exponent.

Measured on the MI355X (printed by the tests), largest err / Y per route and the case it came from; largest
| |w| - 1 |; largest Rayleigh deficit / allowed:
  one workgroup per fold (routes)   1.56  300x33x5x6, Q, component 2 (4.5e-16 against 2.9e-16)   1.83 u   0.000
  one barrier (routes)              1.25  9x33x2x6, Q, component 2 (4.7e-16 against 3.7e-16)     1.62 u   0.000
  four barriers (routes)            0.49  64x448x4x5, Q, component 4 (3.0e-16 against 6.2e-16)   1.32 u   0.000
  M classes, 300x72 / 5x40          1.26 / 1.26  (M = 32, P; M = 2, P)                           1.96 u   0.000
  ladder 5x32x3x10, cond 1e10       1.26  Q, component 9 (4.6e-15 against 3.6e-15)               2.01 u   0.000
  ladder 3x520x3x10                 0.62  cond 1e10, P, component 0                              2.11 u   0.000
  gap ladder, F = 6 / F = 300       0.83 / 0.77  (M = 16, Q; M = 64, B)                          1.81 u   0.001
  zero first entry, F = 6 / 300     1.27 / 1.27  Q, component 2 (5.8e-16 against 4.6e-16)        1.19 u   0.000
  float32 routes, float64 upcast    1.04  9x33x2x6, P, component 5                               1.99 u   0.000
  float32 against float64: |x32 - x64| at most 0.99 x 2^-24 max|x64[a]| (R, 300x24x3x6): the one rounding
The kernels' deficits are at most 0.2 u (the oracle's squaring: 0.5 u); the allowance is dominated by its
64 u |XTY|_F / sigma_1 term (56 u ... 292 u).
Before xreduce summed the slices' parts sixteen at a time as a tree (it was one chain over all slices), route
2x1028x1x4 (S = 115) had | |w| - 1 | = 7.30 u and missed the 4 u bound, with err / Y = 2.28 (Q, component 1:
1.8e-15 against 7.9e-16); a CPU emulation of the chain gives up to 5.6 u on the same fold.  Now 0.98 u and 0.32.
Scratch mutations of the kernel, run once each, and the tests that failed on them: last row dropped from nrm2:
test_follow_routes, test_follow_m_classes (all 29); xreduce without the last slice: test_follow_routes (the four
four-barrier shapes); running B through float: test_follow_routes (all 11); column 0 instead of the largest
diagonal: test_follow_zero_first_entry (both), test_exhaustion_is_exact (5 of 6); no zero-fill beyond n_fit:
test_exhaustion_is_exact (all 6).
The non-finite tests (test_nonfinite_folds, all six cases, and test_nan_fold_end_to_end) fail on the kernel
before the fix: n_fit 0 and zeros for a NaN or an infinity in XTY, one NaN component then zeros for XTX."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pls_cases as pc
from oracle.ikpls_oracle import ikpls_follow

pytestmark = pytest.mark.gpu
U = pc.U
NO_REP = bool(os.environ.get("CVM_PLS_NO_REP"))        # the child of test_four_barrier_kernel_on_small_folds
NO_REP_ROUTE = {(9, 33): pc.ONE, (3, 520): pc.FOUR}    # where the one-barrier shapes of its subset go then
FACTORS = ("B", "W", "P", "Q", "R")


@pytest.fixture(scope="module")
def pls(hip_device):
    assert np.finfo(np.longdouble).eps < 2e-19
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import pls as mod
    return mod


def want_plan(F, K, M, A, dtype, kernel, slices=None, in_lds=None):
    """Every test asserts the route it means to hit."""
    if NO_REP and kernel == pc.REP:
        p = pc.plan(F, K, M, A, dtype)
        assert p["kernel"] == NO_REP_ROUTE.get((F, K), p["kernel"]) != pc.REP, p
        return p
    return pc.assert_plan(F, K, M, A, dtype, kernel, slices, in_lds)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit_np(pls, XTX, XTY, A):
    fit = pls.pls_fit_batched(dev(XTX), dev(XTY), A, return_factors=True)
    assert pls.pls_fit_batched.last_status == 0, "a sliced launch timed out: the device was not idle"
    out = {k: getattr(fit, k).cpu().numpy() for k in FACTORS}
    out["n_fit"] = fit.n_fit.cpu().numpy()
    return out


# ---- follow the weights ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_side(kind, *key):
    """(XTX, XTY, idx, Y, oracle deficit) of a designed case, computed once."""
    if kind == "route":
        F, K, M, A, dtype, cond = key
        XTX, XTY, idx = pc.route_case(F, K, M, A, np.dtype(dtype).type, cond)
    elif kind == "zero":
        F, = key
        A = pc.ZERO_FIRST[2]
        zX, zY = pc.zero_first_case()
        idx = pc.pattern(F, zX.shape[0])
        XTX, XTY = zX[idx], zY[idx]
    else:
        M, F = key
        A = pc.GAP_A
        gX, gY = pc.gap_case(M)
        idx = pc.pattern(F, len(pc.GAPS))
        XTX, XTY = gX[idx], gY[idx]
    first = [int(np.flatnonzero(idx == d)[0]) for d in sorted(set(idx))]
    Y, odef = pc.case_yardstick(XTX[first], XTY[first], A)
    assert np.all(Y <= pc.YARDSTICK_CAP), Y
    for a in (XTX, XTY, idx, Y):
        a.setflags(write=False)
    return XTX, XTY, idx, Y, odef


def check_follow(out, XTX, XTY, idx, A, Y, odef, what):
    """One copy of each distinct matrix against the reference that follows the kernel's weights; the weights
    on their own; every copy bit-identical.  Prints the figures, then asserts."""
    M = XTY.shape[2]
    assert np.all(out["n_fit"] == A), out["n_fit"]
    first = {int(d): int(np.flatnonzero(idx == d)[0]) for d in sorted(set(idx))}
    bad, worst, worst_norm, worst_def = [], (0.0, None), 0.0, (0.0, None)
    for d, f in first.items():
        W = out["W"][f]
        ref = ikpls_follow(XTX[f].astype(np.float64), XTY[f].astype(np.float64), W)
        for a in range(A):
            for name, got, want in (("B", out["B"][f, a], ref[0][a]), ("P", out["P"][f][:, a], ref[1][:, a]),
                                    ("Q", out["Q"][f][:, a], ref[2][:, a]), ("R", out["R"][f][:, a], ref[3][:, a])):
                e = pc.rel(got, want)
                if e / Y[a] > worst[0]:
                    worst = (e / Y[a], f"{name} fold {f} component {a}: {e:.2e} against {Y[a]:.2e}")
                if not e <= pc.gate(Y[a]):
                    bad.append((name, f, a, e, Y[a]))
            w = W[:, a].astype(np.longdouble)
            worst_norm = max(worst_norm, abs(float(np.sqrt(w @ w) - 1)))
        if M > 1:
            defs, slack = pc.deficits(ref[5], W), pc.deficit_slack(XTY[f], ref[5])
            for a in range(A):
                allowed = 2 * odef + slack[a]
                if worst_def[1] is None or defs[a] / allowed > worst_def[0]:
                    worst_def = (defs[a] / allowed, f"fold {f} component {a}: deficit {defs[a] / U:.1f} u, "
                                                    f"oracle {odef / U:.1f} u, allowed {allowed / U:.1f} u")
    print(f"{what}: largest err / Y = {worst[0]:.2f} ({worst[1]}); | |w| - 1 | <= {worst_norm / U:.2f} u; "
          f"deficit / allowed = {worst_def[0]:.3f} ({worst_def[1]})")
    assert not bad, f"{what}: above 2 Y + 4 u: (factor, fold, component, err, Y) " + ", ".join(
        f"({n}, {f}, {a}, {e:.3e}, {y:.3e})" for n, f, a, e, y in bad[:8])
    assert worst_norm <= 4 * U, worst_norm / U
    assert worst_def[0] <= 1.0, worst_def
    for f in range(XTX.shape[0]):
        for k in FACTORS:
            assert pc.same_bits(out[k][f], out[k][first[int(idx[f])]]), (what, k, f)


def route_id(r):
    """9x33x2x6, with the element type where the entry names one that is not float64."""
    tail = [np.dtype(v).name for v in r[4:] if isinstance(v, type) and v is not np.float64]
    return "x".join(str(v) for v in r[:4]) + "".join("-" + t for t in tail)


def ids(cases):
    return [route_id(c) for c in cases]


@pytest.mark.parametrize("route", pc.ROUTES, ids=ids(pc.ROUTES))
def test_follow_routes(pls, route):
    """(a) every route at its smallest shape, ragged slices and the padding blocks of the XCD grid included."""
    F, K, M, A, dtype, kernel, slices, in_lds = route
    want_plan(F, K, M, A, dtype, kernel, slices, in_lds)
    XTX, XTY, idx, Y, odef = reference_side("route", F, K, M, A, "float64", 1e2)
    check_follow(fit_np(pls, XTX, XTY, A), XTX, XTY, idx, A, Y, odef, f"route {route_id(route)} {kernel}")


@pytest.mark.parametrize("M", pc.M_CLASSES)
@pytest.mark.parametrize("F,K,kernel", pc.M_CLASS_ROUTES, ids=[f"{F}x{K}" for F, K, _ in pc.M_CLASS_ROUTES])
def test_follow_m_classes(pls, F, K, kernel, M):
    """(a) the M classes of the eigen code: 1; 1 x 1 and 2 x 2 register blocks; 3 x 3 and 4 x 4 blocks in LDS."""
    want_plan(F, K, M, 3, np.float64, kernel)
    XTX, XTY, idx, Y, odef = reference_side("route", F, K, M, 3, "float64", 1e2)
    check_follow(fit_np(pls, XTX, XTY, 3), XTX, XTY, idx, 3, Y, odef, f"M class {F}x{K}x{M}")


@pytest.mark.parametrize("cond", pc.LADDER_COND, ids=lambda c: f"{c:.0e}")
@pytest.mark.parametrize("F,K,M,A", pc.LADDER_SHAPES, ids=ids(pc.LADDER_SHAPES))
def test_follow_ladder(pls, F, K, M, A, cond):
    """(b) ten components where cond(XTX) is 1e2 ... 1e10: the yardstick grows with it, the gate follows."""
    want_plan(F, K, M, A, np.float64, pc.REP)
    XTX, XTY, idx, Y, odef = reference_side("route", F, K, M, A, "float64", cond)
    check_follow(fit_np(pls, XTX, XTY, A), XTX, XTY, idx, A, Y, odef, f"ladder {F}x{K}x{M}x{A} cond {cond:.0e}")


@pytest.mark.parametrize("F", [6, 300])
@pytest.mark.parametrize("M", pc.GAP_M)
def test_follow_gap_ladder(pls, M, F):
    """(c) leading singular values of XTY a factor sqrt(1 - g) apart, g = 0.5 ... 1e-12 and 0: the squaring runs
    to its cap and the column pick matters.  One fold per gap (F = 6), and the same six among 300."""
    K, A = pc.GAP_K, pc.GAP_A
    want_plan(F, K, M, A, np.float64, pc.REP if F == 6 and M < 64 else pc.ONE)
    XTX, XTY, idx, Y, odef = reference_side("gap", M, F)
    check_follow(fit_np(pls, XTX, XTY, A), XTX, XTY, idx, A, Y, odef, f"gap ladder M={M} F={F}")


@pytest.mark.parametrize("F,kernel", [(6, pc.REP), (300, pc.ONE)], ids=["6", "300"])
def test_follow_zero_first_entry(pls, F, kernel):
    """(c) the column pick: the dominant eigenvector's first entry is exactly zero, so column 0 of the squared
    matrix holds nothing of it (a kernel that took column 0 would extract no component at all); the column of the
    largest diagonal entry does."""
    K, M, A = pc.ZERO_FIRST
    want_plan(F, K, M, A, np.float64, kernel)
    XTX, XTY, idx, Y, odef = reference_side("zero", F)
    out = fit_np(pls, XTX, XTY, A)
    assert np.all(out["Q"][:, 0, 0] == 0)
    check_follow(out, XTX, XTY, idx, A, Y, odef, f"zero first entry F={F}")


F32_ROUTES = [pc.ROUTE_F32, (9, 33, 2, 6, np.float32, pc.REP, 5, False), (300, 24, 3, 6, np.float32, pc.ONE, 1, True)]


@pytest.mark.parametrize("route", F32_ROUTES, ids=ids(F32_ROUTES))
def test_float32_is_the_float64_result_rounded_once(pls, route):
    """The arithmetic is float64 for both element types: the float32 outputs are those of the exact float64
    upcast of the same inputs, rounded once (2^-23 |x|) -- plus 4 u max|x[a]|, the last bit of the float64
    value (the plan depends on the element size, the summation order on the plan) crossing a rounding
    boundary.  The float64 run is held by the follow-the-weights gate."""
    F, K, M, A, dtype, kernel, slices, in_lds = route
    want_plan(F, K, M, A, np.float32, kernel, slices, in_lds)
    XTX, XTY, idx, Y, odef = reference_side("route", F, K, M, A, "float32", 1e2)
    assert XTX.dtype == np.float32
    up = fit_np(pls, XTX.astype(np.float64), XTY.astype(np.float64), A)
    check_follow(up, XTX, XTY, idx, A, Y, odef, f"float32 route {route_id(route)}, upcast")
    lo = fit_np(pls, XTX, XTY, A)
    assert np.array_equal(lo["n_fit"], up["n_fit"])
    for k in FACTORS:
        assert lo[k].dtype == np.float32
        x32, x64 = lo[k].astype(np.float64), up[k]
        ax = (2,) if k != "B" else (1,)                           # components: the last axis, B: the second
        top = np.abs(x64).max(axis=tuple(i for i in range(1, x64.ndim) if i not in ax), keepdims=True)
        excess = np.abs(x32 - x64) - (2.0 ** -23 * np.abs(x64) + 4 * U * top)
        print(f"float32 {route_id(route)} {k}: largest |x32 - x64| = {float((np.abs(x32 - x64) / top).max()) * 2 ** 24:.2f} x 2^-24 max|x64[a]|")
        assert np.all(excess <= 0), (k, float(excess.max()))


# ---- exhaustion --------------------------------------------------------------------------------------------

EXHAUSTION = [(300, 33, 5, 5, pc.ONE), (9, 33, 2, 5, pc.REP), (3, 520, 3, 5, pc.REP), (2, 1028, 1, 5, pc.FOUR),
              (3, 512, 64, 5, pc.FOUR), (64, 448, 4, 5, pc.FOUR)]


@pytest.mark.parametrize("F,K,M,A,kernel", EXHAUSTION, ids=ids(EXHAUSTION))
def test_exhaustion_is_exact(pls, F, K, M, A, kernel):
    """(d) folds of rank 0, 1, 2, 3, 0, ... in one launch, the non-zero rows in the first, a middle and the last
    slice: n_fit is the rank, the extracted components equal the closed form, the others are exactly zero
    (written over a NaN pattern: cabi_fit)."""
    p = want_plan(F, K, M, A, np.float64, kernel)
    XTX, XTY, want = pc.exhaustion_case(F, K, M, A, p["slices"], p["rows"])
    out = cabi_fit(dev(XTX), dev(XTY), A)                         # (outputs prefilled: the zeros have to be written)
    assert np.array_equal(out["n_fit"], want["n_fit"]), out["n_fit"]
    for k in FACTORS:
        got = out[k].reshape(want[k].shape)
        assert np.array_equal(got, want[k]), (k, np.argwhere(got != want[k])[:5])


# ---- non-finite folds --------------------------------------------------------------------------------------

NONFINITE = [(57, 40, 3, 4, np.float64, pc.ONE), (9, 33, 2, 6, np.float64, pc.REP), (3, 520, 3, 4, np.float64, pc.REP),
             (2, 1028, 1, 4, np.float64, pc.FOUR), (3, 512, 64, 5, np.float64, pc.FOUR), (9, 33, 2, 6, np.float32, pc.REP)]


@pytest.mark.parametrize("F,K,M,A,dtype,kernel", NONFINITE, ids=ids(NONFINITE))
def test_nonfinite_folds(pls, F, K, M, A, dtype, kernel):
    """(e) A fold with a NaN or an infinity anywhere in XTX or XTY: B, W, P, Q, R NaN for every component and
    n_fit -1, status 0, and every other fold with the bits it has when that fold is clean.  (Before the fix
    such a fold came out as zeros with n_fit 0, or as one NaN component followed by zeros.)"""
    p = want_plan(F, K, M, A, dtype, kernel)
    XTX, XTY, _ = pc.route_case(F, K, M, A, dtype)
    clean = fit_np(pls, XTX, XTY, A)
    assert np.all(clean["n_fit"] == A) and all(np.all(np.isfinite(clean[k])) for k in FACTORS)
    for i, (name, poke) in enumerate(pc.nonfinite_kinds(K, M, p["slices"], p["rows"])):
        j = (F - 1 - i) % F
        X, Y = XTX.copy(), XTY.copy()
        poke(X[j], Y[j])
        out = fit_np(pls, X, Y, A)                                 # (asserts status 0)
        assert out["n_fit"][j] == -1, (name, j, out["n_fit"])
        for k in FACTORS:
            assert np.all(np.isnan(out[k][j])), (name, k, j, int(np.isfinite(out[k][j]).sum()))
            keep = np.arange(F) != j
            assert pc.same_bits(out[k][keep], clean[k][keep]), (name, k)
        assert np.array_equal(out["n_fit"][keep], clean["n_fit"][keep])


def test_nan_fold_end_to_end(pls):
    """A clean CVMatrix, one fold's training matrices made NaN (what a status-1 fold hands over), the device
    PLS and pls_validation_sse: that fold's errors are NaN for every number of components and the RMSE curve is
    NaN -- never the finite error of predicting the training mean."""
    from cvmatrix_amd import CVMatrix
    from cvmatrix_amd.pls import cv_rmse, pls_validation_sse
    rng = np.random.default_rng(4)
    N, K, M, P, A = 600, 24, 2, 5, 4
    X = rng.standard_normal((N, K))
    Y = X[:, :M] + 0.1 * rng.standard_normal((N, M))
    cvm = CVMatrix(True, True, True, True, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds([np.flatnonzero(np.arange(N) % P == f) for f in range(P)])
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    good = pls.pls_fit_batched(XTX, XTY, A)
    sse0, wsum0 = pls_validation_sse(cvm, batch, stats, good.B)
    assert bool(torch.isfinite(cv_rmse(sse0, wsum0)).all())
    for j, whole in ((2, False), (4, True)):
        X2, Y2 = XTX.clone(), XTY.clone()
        if whole:
            X2[j], Y2[j] = float("nan"), float("nan")
        else:
            Y2[j, K - 1, 0] = float("nan")
        fit = pls.pls_fit_batched(X2, Y2, A)
        assert fit.n_fit.tolist() == [A if f != j else -1 for f in range(P)]
        sse, wsum = pls_validation_sse(cvm, batch, stats, fit.B)
        assert bool(torch.isnan(sse[j]).all())
        keep = [f for f in range(P) if f != j]
        assert torch.equal(sse[keep], sse0[keep]) and torch.equal(wsum, wsum0)
        assert bool(torch.isnan(cv_rmse(sse, wsum)).all())


# ---- buffers, place in the batch, scaling --------------------------------------------------------------------

GUARD = 64
PATTERN = {torch.float64: (torch.int64, 0x7FF8DEAD0000BEEF), torch.float32: (torch.int32, 0x7FC0BEEF),
           torch.int32: (torch.int32, -77)}


def cabi_fit(XTX, XTY, A, optional=True, ws_fill=0x5A):
    """cvm_pls_fit through the C ABI with buffers of its own: every output holds a NaN with a payload (n_fit,
    status: -77) beforehand and has 64 guard elements of the same behind it; the workspace holds `ws_fill` in
    every byte and 64 guard bytes.  Returns the outputs; asserts that every element was written and no guard."""
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, K, M = XTY.shape
    code = _lib.CVM_F64 if XTX.dtype == torch.float64 else _lib.CVM_F32
    nbytes = lib.cvm_pls_workspace_bytes(F, K, M, A, code)
    assert nbytes > 0
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    ws[:nbytes].fill_(ws_fill)
    ws[nbytes:].fill_(0xA5)

    def buf(n, dtype):
        t = torch.empty(n + GUARD, dtype=dtype, device="cuda")
        it, pat = PATTERN[dtype]
        t.view(it).fill_(pat)
        return t

    sizes = {"B": F * A * K * M, "W": F * K * A, "P": F * K * A, "Q": F * M * A, "R": F * K * A}
    bufs = {k: buf(n, XTX.dtype) for k, n in sizes.items() if optional or k == "B"}
    bufs["n_fit"], bufs["status"] = buf(F, torch.int32), buf(1, torch.int32)
    sizes.update(n_fit=F, status=1)
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None     # noqa: E731
    rc = lib.cvm_pls_fit(XTX.data_ptr(), XTY.data_ptr(), F, K, M, A, code, ptr("B"), ptr("W"), ptr("P"), ptr("Q"),
                         ptr("R"), ptr("n_fit"), ptr("status"), ws.data_ptr(), nbytes,
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cvm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace was written past its end"
    out = {}
    for k, t in bufs.items():
        it, pat = PATTERN[t.dtype]
        bits = t.view(it)
        assert bool((bits[sizes[k]:] == pat).all()), f"{k}: written past its end"
        assert not bool((bits[:sizes[k]] == pat).any()), f"{k}: {int((bits[:sizes[k]] == pat).sum())} elements not written"
        out[k] = t[:sizes[k]].cpu().numpy()
    assert out["status"][0] == 0
    return out


BUFFER_SHAPES = [(9, 33, 2, 6, np.float64, pc.REP), (2, 1028, 1, 4, np.float64, pc.FOUR), (300, 33, 5, 6, np.float64, pc.ONE),
                 (9, 33, 2, 6, np.float32, pc.REP)]


@pytest.mark.parametrize("F,K,M,A,dtype,kernel", BUFFER_SHAPES, ids=ids(BUFFER_SHAPES))
def test_outputs_are_written_whole_and_nothing_else(pls, F, K, M, A, dtype, kernel):
    """The outputs and the workspace come from torch.empty: every output element is overwritten (the ragged last
    slice, the padding blocks of the XCD grid), nothing behind an output or the workspace is, the workspace's
    content (0xFF: NaN, 0x7F: huge, 0x00) does not change a bit, with and without the optional outputs."""
    want_plan(F, K, M, A, dtype, kernel)
    XTX, XTY, _ = pc.route_case(F, K, M, A, dtype)
    via_wrapper = fit_np(pls, XTX, XTY, A)
    X, Y = dev(XTX), dev(XTY)
    for fill in (0xFF, 0x7F, 0x00):
        out = cabi_fit(X, Y, A, True, fill)
        for k in FACTORS + ("n_fit",):
            assert pc.same_bits(out[k].reshape(via_wrapper[k].shape), via_wrapper[k]), (fill, k)
        only_b = cabi_fit(X, Y, A, False, fill)
        assert pc.same_bits(only_b["B"], out["B"]) and pc.same_bits(only_b["n_fit"], out["n_fit"]), fill


PLACE_SHAPES = [(9, 33, 2, 6, pc.REP), (300, 24, 3, 6, pc.ONE), (4, 1032, 2, 4, pc.FOUR)]


@pytest.mark.parametrize("F,K,M,A,kernel", PLACE_SHAPES, ids=ids(PLACE_SHAPES))
def test_a_folds_bits_do_not_depend_on_its_place(pls, F, K, M, A, kernel):
    """Distinct matrices, the same F (hence the same plan), the folds permuted: the outputs are the same
    permutation, bit for bit."""
    want_plan(F, K, M, A, np.float64, kernel)
    n = min(F, 9)
    dX, dY = pc.folds(F + K, n, K, M)
    idx = pc.pattern(F, n)
    XTX, XTY = dX[idx], dY[idx]
    out = fit_np(pls, XTX, XTY, A)
    perm = np.random.default_rng(F).permutation(F)
    assert len(set(idx[perm] - idx)) > 1
    moved = fit_np(pls, XTX[perm], XTY[perm], A)
    for k in FACTORS + ("n_fit",):
        assert pc.same_bits(moved[k], out[k][perm]), k


SCALE_SHAPES = [(9, 33, 2, 3, np.float64, pc.REP), (300, 24, 3, 3, np.float64, pc.ONE), (2, 1028, 1, 3, np.float64, pc.FOUR),
                (9, 33, 2, 3, np.float32, pc.REP), (300, 24, 3, 3, np.float32, pc.ONE), (3, 512, 64, 3, np.float32, pc.FOUR)]


@pytest.mark.parametrize("F,K,M,A,dtype,kernel", SCALE_SHAPES, ids=ids(SCALE_SHAPES))
def test_powers_of_two_scale_exactly(pls, F, K, M, A, dtype, kernel):
    """B(2^p XTX, 2^q XTY) == 2^(q - p) B bit for bit and n_fit unchanged: every step scales exactly (the trace
    scaling, the norms -- roots of even powers -- and the divisions), the absolute eps stop is far away."""
    want_plan(F, K, M, A, dtype, kernel)
    XTX, XTY, _ = pc.route_case(F, K, M, A, dtype)
    base = fit_np(pls, XTX, XTY, A)
    assert np.all(base["n_fit"] == A)
    for p, q in ((20, 0), (0, -20), (-20, 20)):
        out = fit_np(pls, XTX * dtype(2.0 ** p), XTY * dtype(2.0 ** q), A)
        assert np.array_equal(out["n_fit"], base["n_fit"]), (p, q)
        assert pc.same_bits(out["B"], base["B"] * dtype(2.0 ** (q - p))), (p, q)
        assert pc.same_bits(out["Q"], base["Q"] * dtype(2.0 ** (q - p))), (p, q)
        for k in ("W", "P", "R"):
            assert pc.same_bits(out[k], base[k]), (p, q, k)


def test_four_barrier_kernel_on_small_folds():
    """CVM_PLS_NO_REP=1 (read once per process, hence a child): the shapes that take the one-barrier route go to
    the four-barrier kernel (K = 520) or to one workgroup per fold (K = 33) -- follow-the-weights on two shapes,
    the non-finite folds and the exhaustion once more there."""
    k = ("((follow_ladder and 3x520) or (follow_routes and 9x33x2x6) or ((nonfinite_folds or exhaustion) and "
         "(9x33 or 3x520))) and not small_folds")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", k],
                       env=dict(os.environ, CVM_PLS_NO_REP="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, r.stdout[-500:]
