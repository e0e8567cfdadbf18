"""CPU: the reference and the gate of tests/predict_cases.py -- the reference against scikit-learn's
PLSRegression.predict and against a plain float64 NumPy evaluation, the gate against a step-by-step NumPy
emulation of the kernel's arithmetic -- and the host half of the device predictions: cvm_cv_predict refuses bad
arguments before the device is touched, cv_predict and predict refuse host tensors."""

import ctypes

import numpy as np
import pytest
import torch

import predict_cases as pc
from cvmatrix_amd import _lib
from cvmatrix_amd import predict as pmod


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_reference_is_sklearn_pls_predict():
    pc.require_longdouble()
    cd = pytest.importorskip("sklearn.cross_decomposition")
    rng = np.random.default_rng(3)
    N, K, M, A = 120, 9, 3, 4
    X = rng.normal(size=(N, K)) * rng.uniform(0.5, 4, K) + rng.normal(size=K)
    Y = X @ rng.normal(size=(K, M)) + 0.1 * rng.normal(size=(N, M)) + 5
    Xn = rng.normal(size=(17, K)) * 2 + 1
    pls = cd.PLSRegression(n_components=A, scale=True).fit(X, Y)
    # the model in this library's terms: coefficients between the standardised sides, and the four statistics
    Bstd = pls.x_rotations_ @ pls.y_loadings_.T
    stats = (X.mean(0), X.std(0, ddof=1), Y.mean(0), Y.std(0, ddof=1))
    ref, gate = pc.reference(Xn, Bstd[None], stats)
    want = pls.predict(Xn)
    assert np.abs(ref[:, 0].astype(np.float64) - want).max() <= 1e-11 * np.abs(want).max()
    assert (gate > 0).all()


def test_reference_is_plain_numpy():
    pc.require_longdouble()
    rng = np.random.default_rng(5)
    for mask in ((True,) * 4, (False,) * 4, (True, False, False, True)):
        X, B, stats = pc.design(rng, 40, 11, 3, 2, np.float64, mask)
        muX, sdX, muY, sdY = stats
        Z = X.copy()
        if muX is not None:
            Z = Z - muX
        if sdX is not None:
            Z = Z / sdX
        want = np.einsum("nk,akm->nam", Z, B)
        if sdY is not None:
            want = want * sdY
        if muY is not None:
            want = want + muY
        ref, gate = pc.reference(X, B, stats)
        assert ref.shape == gate.shape == (40, 3, 2)
        # (the plain evaluation is itself inside the gate: it makes fewer roundings than the kernel)
        assert pc.worst_ratio(want, ref, gate) <= 1.0


@pytest.mark.parametrize("K", [1, 17, 130])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gate_holds_for_an_emulation_of_the_kernel(dtype, K):
    pc.require_longdouble()
    rng = np.random.default_rng(1000 + K)
    worst = 0.0
    for mask in ((True,) * 4, (False,) * 4):
        X, B, stats = pc.design(rng, 129, K, 5, 3, dtype, mask)
        ref, gate = pc.reference(X, B, stats)
        out = pc.emulate(X, B, stats)
        assert out.dtype == np.dtype(dtype)
        worst = max(worst, pc.assert_gate(out, ref, gate, f"emulation {np.dtype(dtype).name} K = {K} {mask}"))
    assert worst > 0.0          # (the gate is not vacuous: the emulation does round)


def test_gate_refuses_a_wrong_result():
    pc.require_longdouble()
    rng = np.random.default_rng(9)
    X, B, stats = pc.design(rng, 20, 17, 2, 3, np.float64)
    ref, gate = pc.reference(X, B, stats)
    out = pc.emulate(X, B, stats)
    out[3, 1, 2] *= 1 + 1e-11              # far outside 2 (K + 8) u, far inside any tolerance by eye
    assert pc.worst_ratio(out, ref, gate) > 1.0


def _call(lib, **kw):
    """cvm_cv_predict with plausible (never dereferenced) arguments, one of them replaced."""
    a = dict(X=4096, ldX=8, idx=4096, offsets=4096, n_folds=2, max_fold_rows=10, K=8, M=3, A=2, dtype=_lib.CVM_F64,
             muX=0, sdX=0, muY=0, sdY=0, B=4096, out=4096, by_row=0, stream=0)
    a.update(kw)
    return lib.cvm_cv_predict(a["X"], a["ldX"], a["idx"], a["offsets"], a["n_folds"], a["max_fold_rows"], a["K"], a["M"],
                              a["A"], a["dtype"], a["muX"], a["sdX"], a["muY"], a["sdY"], a["B"], a["out"], a["by_row"],
                              a["stream"])


@pytest.mark.parametrize("bad", [dict(X=0), dict(offsets=0), dict(B=0), dict(out=0), dict(n_folds=-1),
                                 dict(max_fold_rows=-1), dict(K=0), dict(K=-3), dict(A=0), dict(A=513), dict(M=0),
                                 dict(M=65), dict(ldX=7), dict(dtype=2), dict(dtype=-1), dict(by_row=2),
                                 dict(by_row=-1)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_the_device(lib, bad):
    assert _call(lib, **bad) == _lib.CVM_EINVAL
    assert b"cvm_cv_predict" in lib.cvm_last_error()


def test_no_folds_launch_nothing(lib):
    assert _call(lib, n_folds=0, idx=0) == _lib.CVM_OK


MAX_WGS = 2 ** 32 // 256 - 1      # a launch of 2^32 threads or more in x is refused by the HIP runtime


def plan(lib, F, rows, K, M, A, dtype=_lib.CVM_F64, aligned=1, ldX=None):
    info = np.zeros(9, dtype=np.int64)
    rc = lib.cvm_cv_predict_plan(F, rows, K if ldX is None else ldX, K, M, A, dtype, aligned, info.ctypes.data)
    assert rc == _lib.CVM_OK, lib.cvm_last_error()
    return dict(zip(("nt", "groups", "chunks", "total", "launches", "largest", "lds", "st_in_lds", "vec"), map(int, info)))


@pytest.mark.parametrize("F,rows,A,M", [(1, 1, 1, 1), (10, 10000, 20, 16), (65539, 1, 1, 1), (65539, 16384, 1, 1),
                                        (17_000_000, 1, 1, 1), (2 ** 24 - 1, 64, 1, 1), (2 ** 24, 64, 1, 1),
                                        (2 ** 24, 65, 1, 1), (1, 2 ** 31, 512, 64), (3, 2 ** 36, 1, 1),
                                        (2 ** 40, 1, 1, 1), (70000, 70000, 512, 64), (0, 0, 3, 3), (5, 0, 3, 3)])
@pytest.mark.parametrize("dtype", [_lib.CVM_F64, _lib.CVM_F32])
def test_no_planned_launch_exceeds_the_runtime_limit(lib, dtype, F, rows, A, M):
    """Any number of folds of any length: the flat list of folds x groups x chunks workgroups is covered by
    launches of at most 2^24 - 1 workgroups of 256 threads."""
    p = plan(lib, F, rows, 8, M, A, dtype)
    assert p["chunks"] == max(1, -(-rows // 64)) and p["groups"] == -(-A * M // (64 * p["nt"]))
    assert p["total"] == F * p["groups"] * p["chunks"]
    assert p["largest"] <= MAX_WGS and p["largest"] * 256 < 2 ** 32
    assert p["launches"] == -(-p["total"] // MAX_WGS)
    assert p["largest"] == min(p["total"], MAX_WGS)
    assert p["lds"] <= 160 * 1024


def test_too_much_work_is_refused_not_wrapped(lib):
    info = np.zeros(9, dtype=np.int64)
    for F, rows in ((2 ** 40 + 1, 1), (1, 2 ** 40 + 1), (2 ** 40, 2 ** 40), (2 ** 30, 2 ** 30)):
        assert lib.cvm_cv_predict_plan(F, rows, 8, 8, 1, 1, _lib.CVM_F64, 1, info.ctypes.data) == _lib.CVM_EINVAL
        assert _call(lib, n_folds=F, max_fold_rows=rows) == _lib.CVM_EINVAL


def test_the_routes_the_gpu_tests_mean_to_reach(lib):
    """The plan of the shapes tests/test_gpu_predict.py compares bit for bit: every count of column tiles per
    wave, statistics in and out of LDS, 16-byte loads on and off."""
    f64, f32 = _lib.CVM_F64, _lib.CVM_F32
    assert [plan(lib, 1, 70, 16, 2, c // 2, f64)["nt"] for c in (2, 64, 66, 128, 130, 192, 194, 256, 258, 320, 322)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 3]
    assert [plan(lib, 1, 70, 16, 1, c, f32, aligned=0)["nt"] for c in (320, 321, 384, 385)] == [5, 6, 6, 4]
    assert plan(lib, 1, 70, 17, 8, 41, f64)["nt"] == 3                       # (no 16-byte loads: four tiles at most)
    # statistics: in LDS up to K = 512 under a narrow variant, beyond it only under a wide one
    assert plan(lib, 1, 70, 512, 4, 5, f64)["st_in_lds"] == 1 and plan(lib, 1, 70, 520, 4, 5, f64)["st_in_lds"] == 0
    assert plan(lib, 1, 70, 520, 4, 80, f64) == dict(plan(lib, 1, 70, 520, 4, 80, f64), nt=5, groups=1, st_in_lds=1, vec=1)
    assert plan(lib, 1, 70, 520, 4, 1, f64)["st_in_lds"] == 0
    # 16-byte loads: K, M, the pitch and the addresses
    for K, M, dt, ldX, al, want in ((16, 4, f64, 16, 1, 1), (16, 3, f64, 16, 1, 0), (17, 4, f64, 18, 1, 0), (16, 4, f64, 17, 1, 0),
                                    (16, 4, f64, 16, 0, 0), (2, 2, f64, 2, 1, 0), (36, 16, f32, 36, 1, 1), (34, 4, f32, 34, 1, 0),
                                    (36, 6, f32, 36, 1, 0), (16, 4, f32, 20, 1, 1), (16, 4, f32, 17, 1, 0)):
        assert plan(lib, 1, 70, K, M, 3, dt, al, ldX)["vec"] == want, (K, M, dt, ldX, al)


def test_symbol_is_bound(lib):
    assert "cvm_cv_predict" in _lib.EXPORTS
    assert lib.cvm_cv_predict.restype is ctypes.c_int and len(lib.cvm_cv_predict.argtypes) == 18


def test_host_tensors_are_refused_before_the_device():
    X, B = torch.ones((4, 3), dtype=torch.float64), torch.ones((2, 3, 1), dtype=torch.float64)
    with pytest.raises(TypeError):
        pmod.predict(X, B)
    with pytest.raises(TypeError):
        pmod.predict(X.numpy(), B.numpy())
    with pytest.raises(TypeError):
        pmod.cv_predict(object(), [np.arange(2)], (None,) * 4, B.unsqueeze(0))
    with pytest.raises(TypeError):
        pmod.cv_predict(object(), [np.arange(2)], (None,) * 4, B.unsqueeze(0).numpy())
