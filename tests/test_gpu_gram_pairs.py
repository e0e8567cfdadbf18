"""GPU: the pair map of the LDS-DMA Gram kernel's plain off-diagonal wave (wgram4_body, the WIDE branch, float64).

A lane of that wave takes two adjacent columns of a 32-column group by one 16-byte LDS read and stores two adjacent
columns of a partial by one 16-byte store, so an accumulator's place in the tile is no longer the MFMA's own
(row 32 w + 2 drow + p, column 32 g + 2 lc + q).  A wrong map permutes the off-diagonal tiles of XTX and nothing else,
so every case here has at least one off-diagonal tile and is checked against ``oracle/cvmatrix_oracle.py``.

Through the C ABI, float64: ``cvm_gram_fit`` (ungathered rows, N = 203: the last stage holds 11 rows) and
``cvm_sweep_all`` (gathered rows, three folds of 301 / 260 / 239 rows), for

* K = 256 (one off-diagonal tile), 384 (three), 130 and 254 (the second panel holds 2 / 126 columns: the pairs sit at the
  clamped edge of the loaders' LDS image);
* M = 0, 2, 16;
* weights absent, zero at the first and last row of every row range the plans cut, and negative once;
* the planner's plan and the forced plans 3/5 and 7/2.

Gates: the suite's -- 1e-10 norm-wise for the matrices, rtol 1e-10 for the statistics, XTX and G exactly symmetric.
One float32 case (K = 256, M = 1) shows that its path is what it was (its wave keeps the eight-byte map).

The general kernel (``CVM_FORCE_FALLBACK=1``, read once per process) was compared with the fast path at these shapes on
the commit before the pair map: see ``test_general_kernel_same_bits``."""

import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import assert_normwise, assert_stats, to_np

pytestmark = pytest.mark.gpu

RET_XTX, RET_XTY = 0x01, 0x02
ALL_FLAGS = 0x3F
PLANS = ((0, 0), (3, 5), (7, 2))
FIT_ROWS = (203,)
FOLD_ROWS = (301, 260, 239)
KS = (256, 384, 130, 254)
MS = (0, 2, 16)
WEIGHTS = ("none", "zeros", "negative")
F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvmatrix_amd import _lib

    return _lib, _lib.load(), torch, torch.device("cuda:0")


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
    if kind == "none":
        return None
    parts = []
    for n in sizes:
        w = rng.random(n) + 0.25
        w[_range_edges(n)] = 0.0
        parts.append(w)
    w = np.concatenate(parts)
    if kind == "negative":
        w[sizes[0] // 2 + 1] = -0.5
        assert (w < 0).sum() == 1
    return w.astype(dtype)


@functools.lru_cache(maxsize=None)
def _problem(route, K, M, dtype, kind):
    """Inputs of one case and the oracle's full-data matrices (shared, read-only)."""
    from oracle.cvmatrix_oracle import fit_globals

    sizes = FIT_ROWS if route == "fit" else FOLD_ROWS
    N = sum(sizes)
    rng = np.random.default_rng(100003 * K + 1009 * M + 7 * WEIGHTS.index(kind) + (route == "fit") * 3 + (dtype is F32))
    X = (rng.random((N, K)) + 0.1).astype(dtype)
    Y = (rng.standard_normal((N, M)) + 0.5).astype(dtype) if M else None
    w = _weights(kind, sizes, dtype, rng)
    ref = fit_globals(X.astype(F64), None if Y is None else Y.astype(F64),
                      None if w is None else w.astype(F64).reshape(-1, 1), True, True, True, True)
    for a in (X, Y, w):
        if a is not None:
            a.setflags(write=False)
    return X, Y, w, ref


@functools.lru_cache(maxsize=None)
def _fold_oracle(K, M, dtype, kind):
    """Every fold's training matrices and statistics (float64 oracle; shared, read-only)."""
    from oracle.cvmatrix_oracle import OracleCVMatrix

    X, Y, w, _ = _problem("sweep", K, M, dtype, kind)
    o = OracleCVMatrix()
    o.fit(X.astype(F64), None if Y is None else Y.astype(F64), None if w is None else w.astype(F64))
    offs = np.concatenate([[0], np.cumsum(FOLD_ROWS)])
    out = []
    for f in range(len(FOLD_ROWS)):
        v = np.arange(offs[f], offs[f + 1])
        if M:
            (rx, ry), st = o.training_XTX_XTY(v)
        else:
            (rx, st), ry = o.training_XTX(v), None
        out.append((rx, ry, st))
    return out


def _run_fit(env, K, M, dtype, kind, plan):
    """cvm_gram_fit under `plan`: G, H (None without Y) as NumPy arrays."""
    _lib, lib, torch, dev = env
    X, Y, w, _ = _problem("fit", K, M, dtype, kind)
    N = X.shape[0]
    cdt, tdt = (_lib.CVM_F64, torch.float64) if dtype is F64 else (_lib.CVM_F32, torch.float32)
    Xd = torch.from_numpy(X.copy()).to(dev)
    Yd = None if Y is None else torch.from_numpy(Y.copy()).to(dev)
    wd = None if w is None else torch.from_numpy(w.copy()).to(dev)
    nan = float("nan")
    G = torch.full((K, K), nan, dtype=tdt, device=dev)
    H = torch.full((K, M), nan, dtype=tdt, device=dev) if M else None
    gs = torch.full((int(lib.cvm_gstats_len(K, M)),), nan, dtype=torch.float64, device=dev)
    neg = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.cvm_fit_workspace_bytes(N, K, M, cdt)), dtype=torch.uint8, device=dev)
    assert lib.cvm_debug_force_splits(*plan) == 0
    try:
        rc = lib.cvm_gram_fit(_lib.ptr(Xd), _lib.ptr(Yd), _lib.ptr(wd), N, K, M, cdt, _lib.ptr(G), _lib.ptr(H),
                              _lib.ptr(gs), _lib.ptr(neg), _lib.ptr(ws), ws.numel(), None)
        _lib.check(rc, "cvm_gram_fit")
        torch.cuda.synchronize()
    finally:
        lib.cvm_debug_force_splits(0, 0)
    return {"G": to_np(G), "H": to_np(H), "gstats": to_np(gs)[:2 * K + 2 * M + 2], "neg": to_np(neg)}


def _run_sweep(env, K, M, dtype, kind, plan):
    """cvm_sweep_all under `plan`: every output as a NumPy array."""
    _lib, lib, torch, dev = env
    X, Y, w, _ = _problem("sweep", K, M, dtype, kind)
    P, N = len(FOLD_ROWS), X.shape[0]
    offs = np.concatenate([[0], np.cumsum(FOLD_ROWS)]).astype(np.int64)
    cdt, tdt = (_lib.CVM_F64, torch.float64) if dtype is F64 else (_lib.CVM_F32, torch.float32)
    Xd = torch.from_numpy(X.copy()).to(dev)
    Yd = None if Y is None else torch.from_numpy(Y.copy()).to(dev)
    wd = None if w is None else torch.from_numpy(w.copy()).to(dev)
    idx = torch.arange(N, dtype=torch.int64, device=dev)
    offd = torch.from_numpy(offs.copy()).to(dev)
    nan = float("nan")

    def full(shape, dt=tdt):
        return torch.full(shape, nan, dtype=dt, device=dev)

    o = {"G": full((K, K)), "H": full((K, M)) if M else None,
         "gstats": full((int(lib.cvm_gstats_len(K, M)),), torch.float64),
         "neg": torch.full((1,), -7, dtype=torch.int32, device=dev),
         "XTX": full((P, K, K)), "XTY": full((P, K, M)) if M else None,
         "muX": full((P, 1, K)), "sdX": full((P, 1, K)),
         "muY": full((P, 1, M)) if M else None, "sdY": full((P, 1, M)) if M else None,
         "fold": full((P, 4), torch.float64)}
    ws = torch.empty(int(lib.cvm_sweep_workspace_bytes(P, max(FOLD_ROWS), K, M, cdt)), dtype=torch.uint8, device=dev)
    flags = ALL_FLAGS if M else ALL_FLAGS & ~RET_XTY
    token = C.c_int64(0)
    p = _lib.ptr
    assert lib.cvm_debug_force_splits(*plan) == 0
    try:
        rc = lib.cvm_sweep_all(p(Xd), p(Yd), p(wd), p(idx), p(offd), offs.ctypes.data, P, N, K, M, cdt, flags, 1.0,
                               float(np.finfo(dtype).resolution * 10), p(o["G"]), p(o["H"]), p(o["gstats"]), p(o["neg"]),
                               p(o["XTX"]), p(o["XTY"]) if M else 0, p(o["muX"]), p(o["sdX"]), p(o["muY"]), p(o["sdY"]),
                               p(o["fold"]), p(ws), ws.numel(), None, C.byref(token))
        _lib.check(rc, "cvm_sweep_all")
        torch.cuda.synchronize()
    finally:
        lib.cvm_debug_force_splits(0, 0)
    out = {k: to_np(v) for k, v in o.items()}
    out["gstats"] = out["gstats"][:2 * K + 2 * M + 2]
    return out


def _check_globals(o, ref, K, M, kind, what):
    assert np.array_equal(o["G"], o["G"].T), what + ": G not symmetric"
    assert_normwise(o["G"], ref["G"], 1e-10, what + " G")
    if M:
        assert_normwise(o["H"], ref["H"], 1e-10, what + " H")
    gs = o["gstats"]
    np.testing.assert_allclose(gs[:K], ref["sX"][0], rtol=1e-10, err_msg=what + " sX")
    np.testing.assert_allclose(gs[K:2 * K], ref["qX"][0], rtol=1e-10, err_msg=what + " qX")
    assert int(o["neg"][0]) == int(kind == "negative"), what + " neg_flag"


CASES = [(K, M) for K in KS for M in MS]


@pytest.mark.parametrize("K,M", CASES, ids=[f"K{k}-M{m}" for k, m in CASES])
def test_fit_ungathered(env, K, M):
    """cvm_gram_fit, N = 203, float64: G (exactly symmetric), H and the column sums against the oracle, for the three
    kinds of weights under the three plans."""
    for kind in WEIGHTS:
        ref = _problem("fit", K, M, F64, kind)[3]
        for plan in PLANS:
            o = _run_fit(env, K, M, F64, kind, plan)
            _check_globals(o, ref, K, M, kind, f"fit K={K} M={M} w={kind} plan={plan}")


@pytest.mark.parametrize("K,M", CASES, ids=[f"K{k}-M{m}" for k, m in CASES])
def test_sweep_gathered(env, K, M):
    """cvm_sweep_all over folds of 301 / 260 / 239 gathered rows, float64: the full-data outputs and (no negative
    weight) every fold's matrices and statistics against the oracle; XTX exactly symmetric."""
    for kind in WEIGHTS:
        ref = _problem("sweep", K, M, F64, kind)[3]
        for plan in PLANS:
            what = f"sweep K={K} M={M} w={kind} plan={plan}"
            o = _run_sweep(env, K, M, F64, kind, plan)
            _check_globals(o, ref, K, M, kind, what)
            if kind == "negative":
                continue
            assert np.array_equal(o["XTX"], o["XTX"].transpose(0, 2, 1)), what + ": XTX not symmetric"
            for f, (rx, ry, rst) in enumerate(_fold_oracle(K, M, F64, kind)):
                assert_normwise(o["XTX"][f], rx, 1e-10, f"{what} fold {f} XTX")
                if M:
                    assert_normwise(o["XTY"][f], ry, 1e-10, f"{what} fold {f} XTY")
                got = (o["muX"][f], o["sdX"][f], None if not M else o["muY"][f], None if not M else o["sdY"][f])
                assert_stats(got, rst, 1e-10, f"{what} fold {f}")


def test_float32_path_untouched(env):
    """float32, K = 256, M = 1 (both routes, the planner's plan): the float32 wave keeps its eight-byte map; the
    matrices meet cvmatrix_amd.fp32_gate's bound against the float64 oracle (the yardstick: the oracle's own float32
    error)."""
    from cvmatrix_amd import fp32_gate
    from oracle.cvmatrix_oracle import fit_globals

    K, M = 256, 1
    for route, run in (("fit", _run_fit), ("sweep", _run_sweep)):
        X, Y, w, ref = _problem(route, K, M, F32, "zeros")
        ref32 = fit_globals(X, Y, w.reshape(-1, 1), True, True, True, True)
        o = run(env, K, M, F32, "zeros", (0, 0))
        assert np.array_equal(o["G"], o["G"].T), route + ": G not symmetric"
        for k in ("G", "H"):
            scale = np.abs(ref[k]).max()
            err = np.abs(o[k].astype(F64) - ref[k]).max() / scale
            yard = np.abs(ref32[k].astype(F64) - ref[k]).max() / scale
            print(f"float32 {route} {k}: error {err:.3e}, oracle float32 error {yard:.3e}")
            assert err <= fp32_gate.fp32_bound(yard), f"{route} {k}: error {err:.3e}, oracle float32 error {yard:.3e}"


GENERAL_CASES = [(K, 16, kind) for K in KS for kind in ("none", "zeros")]


def _dump_all(path):
    """(child process of test_general_kernel_same_bits) G, H of the fit and XTX, XTY of the sweep for GENERAL_CASES."""
    import torch
    from cvmatrix_amd import _lib

    e = (_lib, _lib.load(), torch, torch.device("cuda:0"))
    out = {}
    for K, M, kind in GENERAL_CASES:
        a, b = _run_fit(e, K, M, F64, kind, (0, 0)), _run_sweep(e, K, M, F64, kind, (0, 0))
        for k in ("G", "H"):
            out[f"fit-{K}-{kind}-{k}"] = a[k]
        for k in ("G", "H", "XTX", "XTY"):
            out[f"sweep-{K}-{kind}-{k}"] = b[k]
    np.savez(path, **out)


def test_general_kernel_same_bits(env):
    """The general register-staged Gram kernel (CVM_FORCE_FALLBACK=1, read once per process, hence the one child
    process) sums every element in the order of the fast path: on the commit before the pair map the two gave equal
    bits for every array of GENERAL_CASES (K = 256, 384, 130, 254, M = 16, weights absent and zero at the range edges;
    G, H of the fit and G, H, XTX, XTY of the sweep).  The pair map keeps every element's chain, so they still must."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\n"
            f"sys.path[:0] = [{root!r}, {os.path.join(root, 'tests')!r}]\n"
            "import test_gpu_gram_pairs as t\n"
            "t._dump_all(sys.argv[1])\n")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "general.npz")
        subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, CVM_FORCE_FALLBACK="1"),
                       timeout=300)
        general = dict(np.load(path))
    for K, M, kind in GENERAL_CASES:
        a, b = _run_fit(env, K, M, F64, kind, (0, 0)), _run_sweep(env, K, M, F64, kind, (0, 0))
        for route, o, keys in (("fit", a, ("G", "H")), ("sweep", b, ("G", "H", "XTX", "XTY"))):
            for k in keys:
                assert np.array_equal(o[k], general[f"{route}-{K}-{kind}-{k}"]), f"{route} K={K} w={kind}: {k} differs"
