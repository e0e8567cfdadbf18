"""GPU (-m gpu): training matrices of the complements of unions of folds (cvm_sweep_unions through
CVMatrix.training_*_unions) against the oracle on the concatenated validation indices, a golden file from
the reference, the bit contracts of the kernels, float32, the raises, the reuse of the sweep, and the nested
cross-validation example against scikit-learn refits.

Tolerances.  float64: the project's gates, norm-wise 1e-10 for matrices and element-wise 1e-10 for
statistics (the oracle against the naive form is within 3.1e-13 on these designs).  One union of the weighted
design leaves a training set without a non-zero weight: with centring or scaling the reference raises (so does
the library, same message); without, the exact matrices are ZERO and the reference returns the rounding of its
subtraction -- there the 1e-10 gate is taken on the operands of that subtraction, the full-data matrices
(unions_cases.weightless).  float32: the error against
the float64 oracle within fp32_gate.fp32_bound(yardstick), the yardstick being the float32 oracle's own error
on the same union -- the union kernel sums the folds' partials in float64 and adds no rounding of its own."""

import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import unions_cases as uc
from conftest import assert_normwise, assert_stats, golden_stats, load_npz, to_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


@pytest.fixture(scope="module")
def amd(hip_device):
    import cvmatrix_amd
    from cvmatrix_amd import _lib
    _lib.load()
    return cvmatrix_amd


@pytest.fixture
def pad(request, monkeypatch):
    """CVM_PAD=0: the device copies keep the caller's K and M (K = 7: float64 rows that are not 16-byte aligned)."""
    monkeypatch.setenv("CVM_PAD", request.param)
    return request.param


def call(cvm, method, folds, unions):
    return getattr(cvm, f"training_{method}_unions")(folds, unions)


def none_pattern(stats):
    return tuple(s is None for s in stats)


# ---------------------------------------------------------------- 1. float64 parity, every union of the base design
@pytest.mark.parametrize("pad", ["1", "0"], indirect=True)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", uc.SHAPES)
def test_float64_parity_of_every_union(amd, K, M, weighted, pad):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    part = amd.Partitioner(labels)
    order = [int(k) for k in part.folds_dict]                 # position in the batch -> label
    pos = {lab: i for i, lab in enumerate(order)}
    for flags in uc.FLAGS:
        cvm = amd.CVMatrix(*flags, dtype=np.float64)
        cvm.fit(X, Y, w, folds=part)
        for method in (uc.METHODS if M is not None else ("XTX",)):
            refs = uc.base_reference(K, M, weighted, flags, method)
            ok = [u for u, r in enumerate(refs) if not isinstance(r, str)]
            unions = [[pos[f] for f in uc.UNIONS[u]] for u in ok]
            res = call(cvm, method, part, unions)
            gx, gy, gstats = uc.split_result(method, res)
            for i, u in enumerate(ok):
                rx, ry, rstats = uc.split_result(method, refs[u])
                what = f"K={K} M={M} w={weighted} flags={flags} {method} union {uc.UNIONS[u]}"
                if uc.weightless(weighted, uc.UNIONS[u]):
                    # the exact matrices are zero and the reference returns the rounding of total - update: both lie
                    # within the gate taken on the OPERANDS of that subtraction, the full-data matrices
                    sx, sy = uc.full_scale(K, M, weighted)
                    if rx is not None:
                        assert np.abs(to_np(gx[i]) - rx).max() <= TOL * sx, what + " XTX"
                    if ry is not None:
                        assert np.abs(to_np(gy[i]) - ry).max() <= TOL * sy, what + " XTY"
                    assert none_pattern(gstats) == none_pattern(rstats) == (True,) * 4
                    continue
                if rx is not None:
                    assert_normwise(gx[i], rx, TOL, what + " XTX")
                if ry is not None:
                    assert_normwise(gy[i], ry, TOL, what + " XTY")
                assert_stats(tuple(None if s is None else s[i] for s in gstats), rstats, TOL, what)
            assert len(ok) == len(refs) or weighted
            # the unions for which the reference raises: the same message, one union at a time
            for u, r in enumerate(refs):
                if isinstance(r, str):
                    with pytest.raises(ValueError) as e:
                        call(cvm, method, part, [[pos[f] for f in uc.UNIONS[u]]])
                    assert str(e.value) == r


# ---------------------------------------------------------------- 2. the golden file from the reference
@pytest.mark.parametrize("name,flags", [("1111", (True,) * 4), ("0000", (False,) * 4)])
def test_golden_unions(amd, name, flags):
    z = load_npz("g9_unions.npz")
    folds, unions = uc.golden_folds(z), uc.golden_unions(z)
    cvm = amd.CVMatrix(*flags, dtype=np.float64)
    cvm.fit(z["X"], z["Y"], z["w"])
    (xtx, xty), stats = cvm.training_XTX_XTY_unions(folds, unions)
    assert xtx.shape == (11, 5, 5) and xty.shape == (11, 5, 2)
    for u in range(len(unions)):
        assert_normwise(xtx[u], z[f"{name}/{u}/XTX"], TOL, f"{name} union {u} XTX")
        assert_normwise(xty[u], z[f"{name}/{u}/XTY"], TOL, f"{name} union {u} XTY")
        assert_stats(tuple(None if s is None else s[u] for s in stats), golden_stats(z, f"{name}/{u}"), TOL,
                     f"{name} union {u}")


# ---------------------------------------------------------------- 3. bit contracts
def flat(res):
    (a, b), stats = res
    return [a, b] + [s for s in stats if s is not None]


def same_bits(r1, r2, rows1=None, rows2=None):
    t1, t2 = flat(r1), flat(r2)
    assert len(t1) == len(t2)
    for a, b in zip(t1, t2):
        a = a if rows1 is None else a[rows1]
        b = b if rows2 is None else b[rows2]
        # (NaN-free designs: torch.equal is a comparison of the bits up to the sign of zero)
        assert torch.equal(a, b)


@pytest.mark.parametrize("plan", [None, (1, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_union_of_one_fold_has_the_bits_of_the_batched_call(amd, dtype, plan):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    X, Y, w, labels, folds = uc.split_design(np.dtype(dtype).name)
    part = amd.Partitioner(labels)
    try:
        if plan is not None:
            assert lib.cvm_debug_force_splits(*plan) == _lib.CVM_OK
            info = np.zeros(8, dtype=np.int64)
            cvm0 = amd.CVMatrix(dtype=dtype)
            Kd, Md = cvm0._device_dims(X.shape[1], Y.shape[1])
            code = _lib.CVM_F64 if dtype is np.float64 else _lib.CVM_F32
            assert lib.cvm_plan_fold(5, 240, Kd, Md, code, _lib.RET_XTX | _lib.RET_XTY, ctypes.c_size_t(1 << 32),
                                     ctypes.c_void_p(info.ctypes.data)) == _lib.CVM_OK
            assert (int(info[0]), int(info[6])) == plan, info
        for flags in ((True,) * 4, (False,) * 4):
            cvm = amd.CVMatrix(*flags, dtype=dtype)
            cvm.fit(X, Y, w, folds=part)
            ref = cvm.training_XTX_XTY_batched(part)
            got = cvm.training_XTX_XTY_unions(part, [[f] for f in range(5)])
            same_bits(got, ref)
            assert torch.equal(got[0][0], got[0][0].transpose(1, 2))
    finally:
        lib.cvm_debug_force_splits(0, 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_unions_bits_depend_on_its_folds_alone(amd, dtype):
    X, Y, w, labels, folds = uc.base_design(130, 3, True)
    X, Y, w = (a.astype(dtype) for a in (X, Y, w))
    part = amd.Partitioner(labels)
    cvm = amd.CVMatrix(dtype=dtype)
    cvm.fit(X, Y, w, folds=part)
    zero = [i for i, lab in enumerate(part.folds_dict) if int(lab) == 4][0]     # the fold of zero weights
    # (its complement has no non-zero weight: that union raises, test_raises_before_any_launch)
    unions = [S for S in uc.UNIONS if not (len(S) == 4 and zero not in S)]
    everything = cvm.training_XTX_XTY_unions(part, unions)
    xtx = everything[0][0]
    assert torch.equal(xtx, xtx.transpose(1, 2))                         # symmetric to the bit
    for u in (0, 7, 12, len(unions) - 1):
        alone = cvm.training_XTX_XTY_unions(part, [unions[u]])
        same_bits(alone, everything, rows2=slice(u, u + 1))
        cvm._union_ws.fill_(0xFF)                                        # the scratch full of NaN beforehand
        swapped = cvm.training_XTX_XTY_unions(part, [unions[0], unions[u][::-1]])
        same_bits(swapped, everything, rows1=slice(1, 2), rows2=slice(u, u + 1))
    # a list in another order, as an array
    pairs = np.array([S[::-1] for S in unions if len(S) == 2])[::-1].copy()
    idx = [unions.index(sorted(r.tolist())) for r in pairs]
    same_bits(cvm.training_XTX_XTY_unions(part, pairs), everything, rows2=idx)


def test_uncompacted_partials_give_the_same_bits(amd, tmp_path):
    """A child process with CVM_NO_COMPACT=1 (read once per process) writes the pair outputs of a forced-split
    case; this process, whose sweep compacts the folds' partials into slot 0, finds the same bits."""
    from cvmatrix_amd import _lib
    from cvmatrix_amd.unions import fold_pairs
    lib = _lib.load()
    out = str(tmp_path / "pairs.npz")
    env = dict(os.environ, CVM_NO_COMPACT="1", CVM_FORCE_SPLITS="2,3")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "unions_nocompact_check.py"), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert int(z["compacted"]) == 0 and tuple(z["plan"]) == (2, 3)
    X, Y, w, labels, folds = uc.split_design("float64")
    try:
        assert lib.cvm_debug_force_splits(2, 3) == _lib.CVM_OK
        cvm = amd.CVMatrix(dtype=np.float64)
        cvm.fit(X, Y, w, folds=amd.Partitioner(labels))
        assert (cvm._sweep[1] >> 40) & 1 == 1 and cvm._sweep[1] & 0xfffff == 2 and (cvm._sweep[1] >> 20) & 0xfffff == 3
        (xtx, xty), stats = cvm.training_XTX_XTY_unions(cvm.sweep_folds, fold_pairs(5))
    finally:
        lib.cvm_debug_force_splits(0, 0)
    for name, t in zip(("XTX", "XTY", "muX", "sdX", "muY", "sdY"), (xtx, xty) + tuple(stats)):
        assert np.array_equal(to_np(t), z[name]), name


# ---------------------------------------------------------------- 4. float32
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", [(64, 3), (130, 3)])
def test_float32_within_the_reference_float32_error(amd, K, M, weighted):
    from cvmatrix_amd.fp32_gate import fp32_bound
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    c = lambda a: None if a is None else a.astype(np.float32)      # noqa: E731
    part = amd.Partitioner(labels)
    order = [int(k) for k in part.folds_dict]
    pos = {lab: i for i, lab in enumerate(order)}
    for flags in uc.FLAGS:
        ref64 = uc.rounded_reference(K, M, weighted, flags, "XTX_XTY")
        ref32 = uc.base_reference(K, M, weighted, flags, "XTX_XTY", np.float32)
        ok = [u for u, r in enumerate(ref64) if not isinstance(r, str) and not isinstance(ref32[u], str)]
        cvm = amd.CVMatrix(*flags, dtype=np.float32)
        cvm.fit(c(X), c(Y), c(w), folds=part)
        (gx, gy), gstats = cvm.training_XTX_XTY_unions(part, [[pos[f] for f in uc.UNIONS[u]] for u in ok])
        assert gx.dtype == torch.float32 and none_pattern(gstats) == none_pattern(ref64[ok[0]][1])
        for i, u in enumerate(ok):
            for name, got, r64, r32 in (("XTX", gx[i], ref64[u][0][0], ref32[u][0][0]),
                                        ("XTY", gy[i], ref64[u][0][1], ref32[u][0][1])):
                r64 = np.asarray(r64, dtype=np.float64)
                scale = np.abs(r64).max()
                if uc.weightless(weighted, uc.UNIONS[u]):      # (exactly zero matrices: the scale of the operands)
                    scale = uc.full_scale(K, M, weighted, rounded=True)[0 if name == "XTX" else 1]
                err = np.abs(to_np(got).astype(np.float64) - r64).max() / scale
                yard = np.abs(np.asarray(r32, dtype=np.float64) - r64).max() / scale
                assert err <= fp32_bound(yard), (K, weighted, flags, uc.UNIONS[u], name, err, yard)


# ---------------------------------------------------------------- 5. raises
def test_raises_before_any_launch(amd):
    from cvmatrix_amd.cvmatrix import MSG_NZ_DDOF, MSG_NZ_ZERO
    X, Y, w, labels, folds = uc.base_design(64, 3, True)
    part = amd.Partitioner(labels)
    pos = {int(lab): i for i, lab in enumerate(part.folds_dict)}
    nonzero = [pos[f] for f in (0, 1, 2, 3)]                    # fold 4 holds zero weights only
    for flags in ((True, False, False, False), (True,) * 4):
        cvm = amd.CVMatrix(*flags, dtype=np.float64)
        cvm.fit(X, Y, w, folds=part)
        for method in uc.METHODS:
            with pytest.raises(ValueError) as e:
                call(cvm, method, part, [[0], nonzero])
            assert str(e.value) == MSG_NZ_ZERO
        # the per-fold methods on the same rows: the same message
        with pytest.raises(ValueError) as e:
            cvm.training_XTX_XTY(uc.union_indices(folds, (0, 1, 2, 3)))
        assert str(e.value) == MSG_NZ_ZERO
        assert "_union_ws" not in cvm.__dict__                  # nothing was launched: not even the scratch exists
    # without centring and scaling the reference does not look at the counts: no raise
    cvm = amd.CVMatrix(False, False, False, False, dtype=np.float64)
    cvm.fit(X, Y, w, folds=part)
    cvm.training_XTX_XTY_unions(part, [nonzero])
    # ddof: unweighted, the union of folds 0..3 leaves the 22 rows of fold 4
    X, Y, _, labels, folds = uc.base_design(64, 3, False)
    part = amd.Partitioner(labels)
    nonzero = [i for i, lab in enumerate(part.folds_dict) if int(lab) != 4]
    for ddof, raises in ((22, True), (21, False)):
        cvm = amd.CVMatrix(False, False, True, False, ddof=ddof, dtype=np.float64)
        cvm.fit(X, Y, folds=part)
        if raises:
            with pytest.raises(ValueError) as e:
                cvm.training_XTX_unions(part, [[1], nonzero])
            assert str(e.value) == MSG_NZ_DDOF and "_union_ws" not in cvm.__dict__
            with pytest.raises(ValueError) as e:
                cvm.training_XTX(uc.union_indices(folds, (0, 1, 2, 3)))
            assert str(e.value) == MSG_NZ_DDOF
        else:
            cvm.training_XTX_unions(part, [[1], nonzero])
        # centring alone does not need more than one non-zero weight
        amd_c = amd.CVMatrix(True, True, False, False, ddof=ddof, dtype=np.float64)
        amd_c.fit(X, Y, folds=part)
        amd_c.training_XTX_XTY_unions(part, [nonzero])
    # the list of unions
    cvm = amd.CVMatrix(dtype=np.float64)
    cvm.fit(X, Y, folds=part)
    for bad in ([[0, 0]], [[0, 5]], [[-1, 2]], [[1], []], [[]]):
        with pytest.raises(ValueError):
            cvm.training_XTX_XTY_unions(part, bad)
    # folds that are not a partition: the error of fit(folds=...)
    halves = [folds[0], folds[1]]
    with pytest.raises(ValueError) as e1:
        cvm.training_XTX_XTY_unions(halves, [[0, 1]])
    with pytest.raises(ValueError) as e2:
        amd.CVMatrix(dtype=np.float64).fit(X, Y, folds=halves)
    assert str(e1.value) == str(e2.value)
    # Y absent
    cvm = amd.CVMatrix(dtype=np.float64)
    cvm.fit(X, folds=part)
    with pytest.raises(ValueError):
        cvm.training_XTY_unions(part, [[0, 1]])
    with pytest.raises(RuntimeError):
        amd.CVMatrix().training_XTX_unions(part, [[0]])


# ---------------------------------------------------------------- 6. the sweep is reused and not disturbed
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_sweep_is_reused_and_not_disturbed(amd, dtype):
    X, Y, w, labels, folds = uc.base_design(130, 3, True)
    X, Y, w = (a.astype(dtype) for a in (X, Y, w))
    part = amd.Partitioner(labels)
    unions = [[0, 1], [2, 4], [1, 2, 3]]
    plain = amd.CVMatrix(dtype=dtype)
    plain.fit(X, Y, w, folds=part)
    ref_batched = plain.training_XTX_XTY_batched(part)
    cvm = amd.CVMatrix(dtype=dtype)
    cvm.fit(X, Y, w, folds=part)
    token = cvm._sweep
    ref_unions = cvm.training_XTX_XTY_unions(part, unions)
    assert cvm._sweep is token                                       # the partials of fit(folds=...) served the call
    same_bits(cvm.training_XTX_XTY_batched(part), ref_batched)
    same_bits(cvm.training_XTX_XTY_unions(part, unions), ref_unions)
    assert cvm._sweep is token
    # fitted without folds, eager and lazy: the unions call runs the one-sweep fit itself
    for lazy in (False, True):
        other = amd.CVMatrix(dtype=dtype, lazy_fit=lazy)
        other.fit(X, Y, w)
        assert other._sweep is None
        same_bits(other.training_XTX_XTY_unions(part, unions), ref_unions)
        assert other._sweep is not None and not other._pending
        assert torch.equal(other.XTX, cvm.XTX) and torch.equal(other.XTY, cvm.XTY)
        same_bits(other.training_XTX_XTY_batched(part), ref_batched)


# ---------------------------------------------------------------- 7. the example against scikit-learn refits
@pytest.mark.parametrize("weighted", [False, True])
def test_nested_cv_example_against_sklearn_refits(amd, weighted):
    import sklearn.linear_model as lm
    spec = importlib.util.spec_from_file_location("nested_cv_ridge", os.path.join(ROOT, "examples", "nested_cv_ridge.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(5)
    N, K, M, P = 240, 12, 1, 5
    X = rng.standard_normal((N, K))
    Y = X @ rng.standard_normal((K, M)) + 0.5 * rng.standard_normal((N, M)) + 2.0
    w = rng.random(N) + 0.2 if weighted else None
    labels = np.arange(N) % P
    lam = np.array([0.01, 1.0, 50.0])
    res = ex.nested_cv_ridge(X, Y, labels, lam, w)

    def refit_sse(train, val, lv):
        m = lm.Ridge(alpha=lv, fit_intercept=True).fit(X[train], Y[train], None if w is None else w[train])
        wv = np.ones(int(val.sum())) if w is None else w[val]
        pred = np.asarray(m.predict(X[val])).reshape(-1, M)
        return float(wv @ ((pred - Y[val]) ** 2).sum(axis=1)), float(wv.sum())

    inner = np.zeros((P, lam.size))
    for f in range(P):
        wsum = 0.0
        for g in range(P):
            if g == f:
                continue
            for l, lv in enumerate(lam):
                s, ws_ = refit_sse((labels != f) & (labels != g), labels == g, lv)
                inner[f, l] += s
            wsum += ws_
        inner[f] = np.sqrt(inner[f] / (wsum * M))
    np.testing.assert_allclose(res["inner_rmse"], inner, rtol=1e-9)
    assert res["selected"].tolist() == np.argmin(inner, axis=1).tolist()
    outer = np.array([refit_sse(labels != f, labels == f, lam[np.argmin(inner[f])]) for f in range(P)])
    np.testing.assert_allclose(res["outer_sse"][:, 0], outer[:, 0], rtol=1e-9)
    np.testing.assert_allclose(res["outer_wsum"], outer[:, 1], rtol=1e-12)
    np.testing.assert_allclose(res["outer_rmse"], np.sqrt(outer[:, 0].sum() / (outer[:, 1].sum() * M)), rtol=1e-9)
