"""GPU: the Y-side sums of the LDS-DMA Gram kernel's diagonal items (wgram4_diag_body, and ROLE 2 of wgram4_body).

The weights of a range are summed by one compute wave and the non-zero / negative ones COUNTED by it once per
16-row stage (population counts of two compare masks); the Y columns are summed by other waves of the item
(DiagTab::ys / ::ws).  Checked here through the C ABI, where the counts come out as they are:

* ``cvm_gram_fit``: ``gstats`` (``sw``, ``nz``) and ``neg_flag``, N = 203 (the last stage holds 11 rows);
* ``cvm_sweep_all`` over three folds of 301 / 260 / 239 rows: ``out_fold`` = [sw_T, nz_T, sw_V, nz_V] per fold and the
  same full-data outputs,

for K = 128 (one panel) and 256 (a panel that carries the Y sums and one that does not), M = 2 / 16 (one Y tile),
18 (two Y tiles in float64), 40 (a further Y chunk), float32 with M = 1 / 17, with weights that are zero at the first
and last row of every row range the plans cut, zero over a whole stage, negative once, or absent, under the planner's
plan and the forced plans 3/5 and 7/2.  Counts must equal NumPy's exactly; sums and matrices meet the suite's bars
against oracle/cvmatrix_oracle.py (float64 1e-10 norm-wise, statistics rtol 1e-10, float32 through
cvmatrix_amd.fp32_gate under the planner's own plan)."""

import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_normwise, assert_stats, to_np

pytestmark = pytest.mark.gpu

ALL_FLAGS = 0x3F
PLANS = ((0, 0), (3, 5), (7, 2))
FOLD_ROWS = (301, 260, 239)
SHAPES = [(128, 2, np.float64), (128, 16, np.float64), (256, 16, np.float64), (256, 18, np.float64),
          (128, 40, np.float64), (256, 40, np.float64), (128, 1, np.float32), (256, 17, np.float32)]
WEIGHTS = ("zeros", "negative", "none")


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cvmatrix_amd as amd
    from cvmatrix_amd import _lib

    return amd, _lib, _lib.load(), torch, torch.device("cuda:0")


def _range_edges(n):
    """First and last row of every row range a plan of 1 .. 8 splits cuts n rows into (geometry.hpp: split_range)."""
    rows = {0, n - 1}
    for s in range(1, 9):
        per = -(-n // s)
        per = -(-per // 16) * 16
        for sp in range(1, s):
            if sp * per < n:
                rows.update((sp * per - 1, sp * per))
    return sorted(rows)


def _weights(kind, sizes, dtype, rng):
    """One weight vector over the concatenated ranges `sizes`."""
    if kind == "none":
        return None
    parts = []
    for n in sizes:
        w = rng.random(n) + 0.25
        w[_range_edges(n)] = 0.0
        w[32:48] = 0.0                      # a whole stage of zero weights
        w[rng.choice(np.arange(48, n - 1), size=5, replace=False)] = 0.0
        parts.append(w)
    w = np.concatenate(parts)
    if kind == "negative":
        w[sizes[0] // 2 + 1] = -0.5         # exactly one negative weight (never on a zeroed row: odd position past 48)
        assert (w < 0).sum() == 1
    return w.astype(dtype)


@functools.lru_cache(maxsize=None)
def _problem(N_key, K, M, dtype, kind):
    """Inputs and the NumPy / oracle references of one case, computed once and shared (read-only)."""
    from oracle.cvmatrix_oracle import fit_globals

    sizes = (203,) if N_key == "fit" else FOLD_ROWS
    N = sum(sizes)
    rng = np.random.default_rng(K * 1000 + M * 10 + (dtype is np.float32) + 7 * WEIGHTS.index(kind) + (N_key == "fit") * 100000)
    X = (rng.random((N, K)) + 0.1).astype(dtype)
    Y = (rng.standard_normal((N, M)) + 0.5).astype(dtype)
    w = _weights(kind, sizes, dtype, rng)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    w64 = None if w is None else w.astype(np.float64).reshape(-1, 1)
    ref = fit_globals(X64, Y64, w64, True, True, True, True)
    ref32 = None
    if dtype is np.float32:
        ref32 = fit_globals(X, Y, None if w is None else w.reshape(-1, 1), True, True, True, True)
    wv = np.ones(N) if w is None else w.astype(np.float64)
    for a in (X, Y, wv) + (() if w is None else (w,)):
        a.setflags(write=False)
    return X, Y, w, wv, ref, ref32


def _check_globals(_lib, G, H, gs, K, M, dtype, ref, ref32, plan, what):
    from cvmatrix_amd import fp32_gate

    gs = to_np(gs)
    np.testing.assert_allclose(gs[:K], ref["sX"][0], rtol=1e-10 if dtype is np.float64 else 2e-6, err_msg=what + " sX")
    np.testing.assert_allclose(gs[K:2 * K], ref["qX"][0], rtol=1e-10 if dtype is np.float64 else 2e-6, err_msg=what + " qX")
    if dtype is np.float64:
        np.testing.assert_allclose(gs[2 * K:2 * K + M], ref["sY"][0], rtol=0, atol=1e-10 * np.abs(ref["sY"]).max(), err_msg=what + " sY")
        np.testing.assert_allclose(gs[2 * K + M:2 * K + 2 * M], ref["qY"][0], rtol=1e-10, err_msg=what + " qY")
        assert_normwise(G, ref["G"], 1e-10, what + " G")
        assert_normwise(H, ref["H"], 1e-10, what + " H")
    elif plan == (0, 0):
        for got, k in ((G, "G"), (H, "H")):
            scale = np.abs(ref[k]).max()
            err = np.abs(to_np(got).astype(np.float64) - ref[k]).max() / scale
            yard = np.abs(ref32[k].astype(np.float64) - ref[k]).max() / scale
            assert err <= fp32_gate.fp32_bound(yard), f"{what} {k}: error {err:.3e}, reference float32 error {yard:.3e}"


@pytest.mark.parametrize("K,M,dtype", SHAPES, ids=[f"K{k}-M{m}-{'f64' if d is np.float64 else 'f32'}" for k, m, d in SHAPES])
def test_fit_counts_and_sums(env, K, M, dtype):
    """cvm_gram_fit, N = 203: sw, nz, neg_flag (and G, H, the column sums) under the three plans."""
    amd, _lib, lib, torch, dev = env
    cdt = _lib.CVM_F64 if dtype is np.float64 else _lib.CVM_F32
    tdt = torch.float64 if dtype is np.float64 else torch.float32
    try:
        for kind in WEIGHTS:
            X, Y, w, wv, ref, ref32 = _problem("fit", K, M, dtype, kind)
            N = X.shape[0]
            Xd, Yd = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev)
            wd = None if w is None else torch.from_numpy(w.copy()).to(dev)
            for plan in PLANS:
                assert lib.cvm_debug_force_splits(*plan) == 0
                G = torch.full((K, K), float("nan"), dtype=tdt, device=dev)
                H = torch.full((K, M), float("nan"), dtype=tdt, device=dev)
                gs = torch.full((lib.cvm_gstats_len(K, M),), float("nan"), dtype=torch.float64, device=dev)
                neg = torch.full((1,), -7, dtype=torch.int32, device=dev)
                ws = torch.empty(int(lib.cvm_fit_workspace_bytes(N, K, M, cdt)), dtype=torch.uint8, device=dev)
                rc = lib.cvm_gram_fit(Xd.data_ptr(), Yd.data_ptr(), _lib.ptr(wd), N, K, M, cdt, G.data_ptr(), H.data_ptr(),
                                      gs.data_ptr(), neg.data_ptr(), ws.data_ptr(), ws.numel(), None)
                _lib.check(rc, "cvm_gram_fit")
                torch.cuda.synchronize()
                what = f"fit K={K} M={M} {dtype.__name__} w={kind} plan={plan}"
                g = to_np(gs)
                print(what, "sw", g[2 * K + 2 * M], "nz", g[2 * K + 2 * M + 1], "neg", int(neg.item()))
                assert g[2 * K + 2 * M + 1] == float(np.count_nonzero(wv)), what + " nz"
                assert int(neg.item()) == int((wv < 0).any()), what + " neg_flag"
                np.testing.assert_allclose(g[2 * K + 2 * M], wv.sum(), rtol=1e-10, err_msg=what + " sw")
                _check_globals(_lib, G, H, gs, K, M, dtype, ref, ref32, plan, what)
    finally:
        lib.cvm_debug_force_splits(0, 0)


@pytest.mark.parametrize("K,M,dtype", SHAPES, ids=[f"K{k}-M{m}-{'f64' if d is np.float64 else 'f32'}" for k, m, d in SHAPES])
def test_sweep_counts_and_sums(env, K, M, dtype):
    """cvm_sweep_all over folds of 301 / 260 / 239 rows: out_fold's sums and counts per fold, the full-data
    outputs, and (float64, no negative weight) every fold's matrices and statistics against the oracle."""
    from oracle.cvmatrix_oracle import OracleCVMatrix

    amd, _lib, lib, torch, dev = env
    cdt = _lib.CVM_F64 if dtype is np.float64 else _lib.CVM_F32
    tdt = torch.float64 if dtype is np.float64 else torch.float32
    P = len(FOLD_ROWS)
    offs = np.concatenate([[0], np.cumsum(FOLD_ROWS)]).astype(np.int64)
    N = int(offs[-1])
    try:
        for kind in WEIGHTS:
            X, Y, w, wv, ref, ref32 = _problem("sweep", K, M, dtype, kind)
            Xd, Yd = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev)
            wd = None if w is None else torch.from_numpy(w.copy()).to(dev)
            idx = torch.arange(N, dtype=torch.int64, device=dev)
            offd = torch.from_numpy(offs.copy()).to(dev)
            oracle = None
            if dtype is np.float64 and kind != "negative":
                oracle = OracleCVMatrix()
                oracle.fit(X, Y, w)
                oref = [(oracle.training_XTX_XTY(np.arange(offs[f], offs[f + 1]))) for f in range(P)]
            for plan in PLANS:
                assert lib.cvm_debug_force_splits(*plan) == 0
                G = torch.full((K, K), float("nan"), dtype=tdt, device=dev)
                H = torch.full((K, M), float("nan"), dtype=tdt, device=dev)
                gs = torch.full((lib.cvm_gstats_len(K, M),), float("nan"), dtype=torch.float64, device=dev)
                neg = torch.full((1,), -7, dtype=torch.int32, device=dev)
                oX = torch.full((P, K, K), float("nan"), dtype=tdt, device=dev)
                oY = torch.full((P, K, M), float("nan"), dtype=tdt, device=dev)
                muX, sdX = torch.empty((P, 1, K), dtype=tdt, device=dev), torch.empty((P, 1, K), dtype=tdt, device=dev)
                muY, sdY = torch.empty((P, 1, M), dtype=tdt, device=dev), torch.empty((P, 1, M), dtype=tdt, device=dev)
                of = torch.full((P, 4), float("nan"), dtype=torch.float64, device=dev)
                ws = torch.empty(int(lib.cvm_sweep_workspace_bytes(P, max(FOLD_ROWS), K, M, cdt)), dtype=torch.uint8, device=dev)
                token = C.c_int64(0)
                rc = lib.cvm_sweep_all(Xd.data_ptr(), Yd.data_ptr(), _lib.ptr(wd), idx.data_ptr(), offd.data_ptr(),
                                       offs.ctypes.data, P, N, K, M, cdt, ALL_FLAGS, 1.0, float(np.finfo(dtype).resolution * 10),
                                       G.data_ptr(), H.data_ptr(), gs.data_ptr(), neg.data_ptr(), oX.data_ptr(), oY.data_ptr(),
                                       muX.data_ptr(), sdX.data_ptr(), muY.data_ptr(), sdY.data_ptr(), of.data_ptr(),
                                       ws.data_ptr(), ws.numel(), None, C.byref(token))
                _lib.check(rc, "cvm_sweep_all")
                torch.cuda.synchronize()
                what = f"sweep K={K} M={M} {dtype.__name__} w={kind} plan={plan}"
                g, o = to_np(gs), to_np(of)
                print(what, "out_fold", o.tolist(), "nz", g[2 * K + 2 * M + 1], "neg", int(neg.item()))
                assert g[2 * K + 2 * M + 1] == float(np.count_nonzero(wv)), what + " nz"
                assert int(neg.item()) == int((wv < 0).any()), what + " neg_flag"
                np.testing.assert_allclose(g[2 * K + 2 * M], wv.sum(), rtol=1e-10, err_msg=what + " sw")
                for f in range(P):
                    v = wv[offs[f]:offs[f + 1]]
                    assert o[f, 3] == float(np.count_nonzero(v)), f"{what} fold {f} nz_V"
                    assert o[f, 1] == float(np.count_nonzero(wv) - np.count_nonzero(v)), f"{what} fold {f} nz_T"
                    np.testing.assert_allclose(o[f, 2], v.sum(), rtol=1e-10, err_msg=f"{what} fold {f} sw_V")
                    np.testing.assert_allclose(o[f, 0], wv.sum() - v.sum(), rtol=1e-10, err_msg=f"{what} fold {f} sw_T")
                _check_globals(_lib, G, H, gs, K, M, dtype, ref, ref32, plan, what)
                if oracle is not None:
                    for f in range(P):
                        (rx, ry), rst = oref[f]
                        assert_normwise(oX[f], rx, 1e-10, f"{what} fold {f} XTX")
                        assert_normwise(oY[f], ry, 1e-10, f"{what} fold {f} XTY")
                        assert_stats((muX[f], sdX[f], muY[f], sdY[f]), rst, 1e-10, f"{what} fold {f}")
    finally:
        lib.cvm_debug_force_splits(0, 0)


@pytest.mark.parametrize("dtype,M", [(np.float64, 16), (np.float64, 18), (np.float32, 17)])
def test_weighted_constant_one_columns_have_std_exactly_one(env, dtype, M):
    """A weighted constant-one column of X (summed by the waves of its panel) and of Y (summed by the waves the
    table names) has s == q == sw bit for bit, so its variance is exactly zero and the public API returns std 1."""
    amd, _lib, lib, torch, dev = env
    rng = np.random.default_rng(99)
    N, K, P = sum(FOLD_ROWS), 256, len(FOLD_ROWS)
    X = rng.random((N, K)).astype(dtype)
    Y = rng.random((N, M)).astype(dtype)
    X[:, 3] = 1.0
    X[:, 200] = 1.0
    Y[:, 0] = 1.0
    Y[:, M - 1] = 1.0
    w = (rng.random(N) + 0.25).astype(dtype)
    w[::7] = 0.0
    labels = np.repeat(np.arange(P), FOLD_ROWS)
    try:
        for plan in PLANS:
            assert lib.cvm_debug_force_splits(*plan) == 0
            for lazy in (True, False):
                m = amd.CVMatrix(dtype=dtype, lazy_fit=lazy)
                m.fit(X, Y, w)
                _, (muX, sdX, muY, sdY) = m.training_XTX_XTY_batched(amd.Partitioner(labels))
                sx, sy = to_np(sdX).reshape(P, K), to_np(sdY).reshape(P, M)
                what = f"{dtype.__name__} M={M} plan={plan} lazy={lazy}"
                assert (sx[:, [3, 200]] == 1.0).all(), what + f" sdX {sx[:, [3, 200]]}"
                assert (sy[:, [0, M - 1]] == 1.0).all(), what + f" sdY {sy[:, [0, M - 1]]}"
                assert (to_np(muX).reshape(P, K)[:, [3, 200]] == 1.0).all(), what + " muX"
    finally:
        lib.cvm_debug_force_splits(0, 0)
