"""GPU: the one-launch finalize of the one-sweep path (``sweep_finalize_kernel``, finalize.hpp), through the C ABI.

``cvm_sweep_all`` takes it for at most 16 folds, 16-byte aligned rows and aligned ``G`` / ``out_XTX``.  Every
workgroup of that launch forms the fold statistics of the columns it touches itself and designated workgroups
write the statistics buffers, so the checks here are

1. bit equality of every output with ``cvm_sweep_fit`` + ``cvm_sweep_folds`` on the same workspace (the route
   ``CVM_NO_SWEEP_MERGE`` selects: ``fit_apply_kernel``, ``fold_stats_kernel``, ``apply_kernel``), every output buffer
   poisoned with NaN before each call so that a piece nobody wrote shows;
2. the oracle (oracle/cvmatrix_oracle.py) at the suite's gates: 1e-10 norm-wise in float64, ``fp32_bound`` of the
   oracle's own float32 error in float32; every XTX exactly symmetric;
3. the same bits from a second call, and from 50 calls of the case with the most entries;
4. every element of the statistics buffers written (K = 264, M = 33, P = 5).

The shapes are the smallest at which each index expression of the kernel can go wrong: K = 16 (one block), 40 (a
ragged block inside one tile), 128 (a full tile), 136 (a tile plus 8 columns), 264 (three panels with ragged
off-diagonal tiles) in float64 and 36 / 132 / 264 in float32 (multiples of 4, not of 32); M = 0, 1, 16, 33; 2, 3, 5,
10 and 16 folds (3 and 5 are not multiples of the four fold groups; 16 is the most the kernel takes) of 300 rows;
17 folds and an odd K must still take the separate kernels.  Forced plans (1, 1), (3, 9) -- a second group of eight
partials -- and (5, 2) -- the slot stride is s_off -- run on folds of 640 rows, which those split counts fit."""

import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_normwise, to_np

pytestmark = pytest.mark.gpu

RET_XTX, RET_XTY = 0x01, 0x02
ALL_FLAGS = 0x3F
F64, F32 = np.float64, np.float32
# dtype, K, M, folds, weighted
CASES = [
    (F64, 16, 1, 2, True), (F64, 40, 0, 3, False), (F64, 40, 33, 16, False), (F64, 128, 16, 5, True),
    (F64, 128, 1, 3, False), (F64, 136, 33, 10, False), (F64, 264, 33, 5, True), (F64, 264, 16, 16, True),
    (F32, 36, 1, 3, True), (F32, 36, 0, 5, False), (F32, 132, 16, 10, False), (F32, 264, 33, 16, True),
]
OUTPUTS = ("G", "H", "gstats", "neg", "XTX", "XTY", "muX", "sdX", "muY", "sdY", "fold")


def _id(c):
    return f"{'f64' if c[0] is F64 else 'f32'}-K{c[1]}-M{c[2]}-P{c[3]}-{'w' if c[4] else 'u'}"


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvmatrix_amd import _lib

    return _lib, _lib.load(), torch, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _problem(dtype, K, M, P, weighted, rows=300):
    """Inputs of one case (read-only, shared): P folds of `rows` consecutive rows."""
    N = rows * P
    rng = np.random.default_rng(100003 * K + 1009 * M + 17 * P + weighted + (dtype is F32) * 7)
    X = (rng.random((N, K)) + 0.1).astype(dtype)
    Y = (rng.standard_normal((N, M)) + 0.5).astype(dtype) if M else None
    w = None
    if weighted:
        w = rng.random(N) + 0.25
        w[::13] = 0.0
        w = w.astype(dtype)
    offs = (np.arange(P + 1) * rows).astype(np.int64)
    for a in (X, Y, w, offs):
        if a is not None:
            a.setflags(write=False)
    return X, Y, w, offs


@functools.lru_cache(maxsize=None)
def _oracle(dtype, K, M, P, weighted, flags, odtype, rows=300):
    """Every fold's training matrices and statistics by the oracle computing in `odtype` (shared, read-only)."""
    from oracle.cvmatrix_oracle import OracleCVMatrix

    X, Y, w, offs = _problem(dtype, K, M, P, weighted, rows)
    o = OracleCVMatrix(bool(flags & 4), bool(flags & 8), bool(flags & 16), bool(flags & 32), 1, odtype)
    o.fit(X.astype(odtype), None if Y is None else Y.astype(odtype), None if w is None else w.astype(odtype))
    out = []
    for f in range(P):
        v = np.arange(offs[f], offs[f + 1])
        rx = ry = None
        if M and flags & RET_XTX and flags & RET_XTY:
            (rx, ry), st = o.training_XTX_XTY(v)
        elif M and flags & RET_XTY:
            ry, st = o.training_XTY(v)
        else:       # XTX only -- or neither: the statistics the library then forms are those of an XTX call
            rx, st = o.training_XTX(v)
            if not flags & RET_XTX:
                rx = None
        out.append((rx, ry, st))
    return out


class _Device:
    """The inputs of a case on the device, and the two routes over them."""

    def __init__(self, env, dtype, K, M, P, weighted, rows=300):
        self._lib, self.lib, self.torch, self.dev = env
        torch, dev = self.torch, self.dev
        self.dtype, self.K, self.M, self.P, self.rows = dtype, K, M, P, rows
        X, Y, w, offs = _problem(dtype, K, M, P, weighted, rows)
        self.N = X.shape[0]
        self.offs = offs.copy()
        self.Xd = torch.from_numpy(X.copy()).to(dev)
        self.Yd = None if Y is None else torch.from_numpy(Y.copy()).to(dev)
        self.wd = None if w is None else torch.from_numpy(w.copy()).to(dev)
        self.idx = torch.arange(self.N, dtype=torch.int64, device=dev)
        self.offd = torch.from_numpy(self.offs).to(dev)
        self.cdt = self._lib.CVM_F64 if dtype is F64 else self._lib.CVM_F32
        self.tdt = torch.float64 if dtype is F64 else torch.float32
        self.ws = torch.empty(int(self.lib.cvm_sweep_workspace_bytes(P, rows, K, M, self.cdt)), dtype=torch.uint8, device=dev)

    def poisoned(self):
        torch, dev, K, M, P = self.torch, self.dev, self.K, self.M, self.P
        nan = float("nan")
        o = {"G": torch.full((K, K), nan, dtype=self.tdt, device=dev),
             "H": torch.full((K, M), nan, dtype=self.tdt, device=dev) if M else None,
             "gstats": torch.full((int(self.lib.cvm_gstats_len(K, M)),), nan, dtype=torch.float64, device=dev),
             "neg": torch.full((1,), -7, dtype=torch.int32, device=dev),
             "XTX": torch.full((P, K, K), nan, dtype=self.tdt, device=dev),
             "XTY": torch.full((P, K, M), nan, dtype=self.tdt, device=dev) if M else None,
             "muX": torch.full((P, K), nan, dtype=self.tdt, device=dev),
             "sdX": torch.full((P, K), nan, dtype=self.tdt, device=dev),
             "muY": torch.full((P, M), nan, dtype=self.tdt, device=dev) if M else None,
             "sdY": torch.full((P, M), nan, dtype=self.tdt, device=dev) if M else None,
             "fold": torch.full((P, 4), nan, dtype=torch.float64, device=dev)}
        return o

    def run(self, route, flags=ALL_FLAGS):
        """route "one": cvm_sweep_all; "two": cvm_sweep_fit + cvm_sweep_folds.  Returns the outputs (device) and the
        plan token."""
        _lib, lib, P, K, M = self._lib, self.lib, self.P, self.K, self.M
        if not M:
            flags &= ~RET_XTY
        o = self.poisoned()
        p = _lib.ptr
        res = float(np.finfo(self.dtype).resolution * 10)
        token = C.c_int64(0)
        oX = p(o["XTX"]) if flags & RET_XTX else 0
        oY = p(o["XTY"]) if flags & RET_XTY else 0
        if route == "one":
            rc = lib.cvm_sweep_all(p(self.Xd), p(self.Yd), p(self.wd), p(self.idx), p(self.offd), self.offs.ctypes.data,
                                   P, self.N, K, M, self.cdt, flags, 1.0, res, p(o["G"]), p(o["H"]), p(o["gstats"]),
                                   p(o["neg"]), oX, oY, p(o["muX"]), p(o["sdX"]), p(o["muY"]), p(o["sdY"]), p(o["fold"]),
                                   p(self.ws), self.ws.numel(), None, C.byref(token))
            _lib.check(rc, "cvm_sweep_all")
        else:
            rc = lib.cvm_sweep_fit(p(self.Xd), p(self.Yd), p(self.wd), p(self.idx), p(self.offd), self.offs.ctypes.data,
                                   P, self.N, K, M, self.cdt, p(o["G"]), p(o["H"]), p(o["gstats"]), p(o["neg"]),
                                   p(self.ws), self.ws.numel(), None, C.byref(token))
            _lib.check(rc, "cvm_sweep_fit")
            rc = lib.cvm_sweep_folds(p(self.offd), P, K, M, self.cdt, flags, 1.0, res, int(self.wd is not None),
                                     p(o["G"]), p(o["H"]), p(o["gstats"]), oX, oY, p(o["muX"]), p(o["sdX"]), p(o["muY"]),
                                     p(o["sdY"]), p(o["fold"]), p(self.ws), self.ws.numel(), token.value, None)
            _lib.check(rc, "cvm_sweep_folds")
        self.torch.cuda.synchronize()
        return o, token.value


def _same_bits(a, b, what, n_gstats):
    """Every output of two runs, bit for bit (poison that both left counts as equal: NaN has one pattern here)."""
    for k in OUTPUTS:
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = to_np(a[k]), to_np(b[k])
        if k == "gstats":
            x, y = x[:n_gstats], y[:n_gstats]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {k} differs"


def _norm_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(to_np(got).astype(np.float64).reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _against_oracle(dv, o, flags, weighted, what, plan=None):
    """The folds' matrices (those the flags ask for) and statistics against the oracle; XTX exactly symmetric.
    float32: cvmatrix_amd.fp32_gate's rule -- twice the oracle's own float32 error plus two roundings of the scale,
    and one more per partial a forced plan adds to a tile (the gate reads a forced plan from the environment only,
    so a plan forced through cvm_debug_force_splits is added here, by the same rule: max(plan) - 1)."""
    from cvmatrix_amd import fp32_gate

    def bound(yard):
        return fp32_gate.fp32_bound(yard) + ((max(plan) - 1) * fp32_gate.FP32_EPS if plan else 0.0)

    dtype, K, M, P = dv.dtype, dv.K, dv.M, dv.P
    if not M:
        flags &= ~RET_XTY
    ref = _oracle(dtype, K, M, P, weighted, flags, F64, dv.rows)
    ref32 = _oracle(dtype, K, M, P, weighted, flags, F32, dv.rows) if dtype is F32 else None
    if flags & RET_XTX:
        xtx = to_np(o["XTX"])
        assert np.array_equal(xtx, xtx.transpose(0, 2, 1)), what + ": XTX not symmetric"
    g = to_np(o["G"])
    assert np.array_equal(g, g.T), what + ": G not symmetric"
    for f in range(P):
        rx, ry, rst = ref[f]
        pairs = ([("XTX", o["XTX"][f], rx, 0)] if rx is not None else []) + ([("XTY", o["XTY"][f], ry, 1)] if ry is not None else [])
        for name, got, r, i in pairs:
            if dtype is F64:
                assert_normwise(got, r, 1e-10, f"{what} fold {f} {name}")
            else:
                err, yard = _norm_err(got, r), _norm_err(ref32[f][i], r)
                print(f"{what} fold {f} {name}: error {err:.3e}, oracle float32 error {yard:.3e}")
                assert err <= bound(yard), f"{what} fold {f} {name}: {err:.3e} > bound of {yard:.3e}"
        for i, name in enumerate(("muX", "sdX", "muY", "sdY")):
            if rst[i] is None:
                continue
            if dtype is F64:
                np.testing.assert_allclose(to_np(o[name][f]).reshape(-1), np.asarray(rst[i]).reshape(-1), rtol=1e-10, atol=0,
                                           err_msg=f"{what} fold {f} {name}")
            else:
                err, yard = _norm_err(o[name][f], rst[i]), _norm_err(ref32[f][2][i], rst[i])
                assert err <= bound(yard), f"{what} fold {f} {name}: {err:.3e} > bound of {yard:.3e}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_one_launch_equals_separate_kernels_and_oracle(env, case):
    """Every output of cvm_sweep_all bit-equal to cvm_sweep_fit + cvm_sweep_folds and to a second call; the folds
    against the oracle."""
    dtype, K, M, P, weighted = case
    dv = _Device(env, dtype, K, M, P, weighted)
    n_gs = 2 * K + 2 * M + 2
    one, _ = dv.run("one")
    again, _ = dv.run("one")
    two, _ = dv.run("two")
    _same_bits(one, two, _id(case) + " one launch / separate kernels", n_gs)
    _same_bits(one, again, _id(case) + " second call", n_gs)
    assert not np.isnan(to_np(one["gstats"])[:n_gs]).any() and not np.isnan(to_np(one["fold"])).any()
    _against_oracle(dv, one, ALL_FLAGS & (~RET_XTY if not M else ~0), weighted, _id(case))


@pytest.mark.parametrize("case", [(F64, 40, 3, 17, True), (F64, 135, 16, 4, True), (F64, 33, 1, 3, False)], ids=_id)
def test_more_folds_or_unaligned_rows_take_the_separate_kernels(env, case):
    """17 folds, or rows that are no multiple of 16 bytes: the same entry point, the separate kernels, the oracle."""
    dtype, K, M, P, weighted = case
    dv = _Device(env, dtype, K, M, P, weighted)
    one, _ = dv.run("one")
    two, _ = dv.run("two")
    _same_bits(one, two, _id(case), 2 * K + 2 * M + 2)
    _against_oracle(dv, one, ALL_FLAGS, weighted, _id(case))


def test_every_centre_scale_combination(env):
    """All 16 combinations of centre / scale X / Y on K = 136, M = 33, three folds, weighted."""
    case = (F64, 136, 33, 3, True)
    dv = _Device(env, *case)
    for cs in range(16):
        flags = RET_XTX | RET_XTY | (cs << 2)
        one, _ = dv.run("one", flags)
        two, _ = dv.run("two", flags)
        _same_bits(one, two, f"flags {flags:#x}", 2 * 136 + 2 * 33 + 2)
        _against_oracle(dv, one, flags, True, f"flags {flags:#x}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_one_kind_of_output_only(env, dtype):
    """XTX only, XTY only, statistics only (out_XTX == NULL leaves the one output G)."""
    K, M, P = 264, 33, 5
    dv = _Device(env, dtype, K, M, P, True)
    for ret in (RET_XTX, RET_XTY, 0):
        flags = (ALL_FLAGS & ~3) | ret
        one, _ = dv.run("one", flags)
        two, _ = dv.run("two", flags)
        _same_bits(one, two, f"{dtype.__name__} ret {ret}", 2 * K + 2 * M + 2)
        assert not np.isnan(to_np(one["G"])).any() and not np.isnan(to_np(one["H"])).any()
        assert np.isnan(to_np(one["XTX"])).all() == (not ret & RET_XTX)
        assert np.isnan(to_np(one["XTY"])).all() == (not ret & RET_XTY)
        _against_oracle(dv, one, flags, True, f"{dtype.__name__} ret {ret}")


@pytest.mark.parametrize("plan", [(1, 1), (3, 9), (5, 2)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_forced_plans(env, plan):
    """Row-split plans the planner would not pick, folds of 640 rows (which take up to ten splits)."""
    _lib, lib, torch, dev = env
    try:
        assert lib.cvm_debug_force_splits(*plan) == 0
        for dtype, K, M, P, weighted in ((F64, 264, 33, 3, True), (F32, 264, 16, 5, False)):
            dv = _Device(env, dtype, K, M, P, weighted, rows=640)
            one, token = dv.run("one")
            assert (token & 0xfffff, (token >> 20) & 0xfffff) == plan, "the forced plan was not taken"
            two, _ = dv.run("two")
            again, _ = dv.run("one")
            what = f"plan {plan} {dtype.__name__}"
            _same_bits(one, two, what, 2 * K + 2 * M + 2)
            _same_bits(one, again, what + " second call", 2 * K + 2 * M + 2)
            _against_oracle(dv, one, ALL_FLAGS, weighted, what, plan)
    finally:
        lib.cvm_debug_force_splits(0, 0)


def test_fifty_calls_give_the_same_bits(env):
    """K = 264, 16 folds (the case with the most entries and the largest LDS image), 50 calls."""
    _lib, lib, torch, dev = env
    dv = _Device(env, F64, 264, 16, 16, True)
    first, _ = dv.run("one")
    for i in range(50):
        o, _ = dv.run("one")
        for k in OUTPUTS:
            a, b = o[k], first[k]
            if k == "gstats":       # (behind its 2 K + 2 M + 2 entries the buffer keeps its poison)
                a, b = a[:2 * 264 + 2 * 16 + 2], b[:2 * 264 + 2 * 16 + 2]
            assert torch.equal(a, b), f"call {i}: {k} differs"
    assert not torch.isnan(first["gstats"][:2 * 264 + 2 * 16 + 2]).any() and int(first["neg"].item()) == 0


def test_every_statistic_has_a_writer(env):
    """K = 264, M = 33, 5 folds: every element of the statistics outputs, out_fold and gstats is written, with the
    separate kernels' values."""
    K, M, P = 264, 33, 5
    for dtype, weighted in ((F64, True), (F32, False)):
        dv = _Device(env, dtype, K, M, P, weighted)
        one, _ = dv.run("one")
        two, _ = dv.run("two")
        for k in ("muX", "sdX", "muY", "sdY", "fold"):
            a = to_np(one[k])
            assert not np.isnan(a).any(), f"{dtype.__name__} {k}: elements nobody wrote"
            assert np.array_equal(a, to_np(two[k])), f"{dtype.__name__} {k}"
        gs = to_np(one["gstats"])[:2 * K + 2 * M + 2]
        assert not np.isnan(gs).any(), "gstats: elements nobody wrote"
        assert np.array_equal(gs, to_np(two["gstats"])[:2 * K + 2 * M + 2])
        assert int(one["neg"].item()) == int(two["neg"].item()) == 0
