"""GPU (-m gpu): the HIP path, called through the C ABI of libcvmhip.so, against
(1) the golden vectors produced by the reference, (2) the CPU oracle on the same seeded
inputs, and (3) size-independent properties at BASELINE.json's full shapes.

Tolerance: fp64 norm-wise 1e-10 (max|d| <= 1e-10 max|ref| and
Frobenius), statistics element-wise rtol 1e-10.  fp32: compared with the fp64 reference;
error must not exceed 2x the reference's own float32 error (stored with the digests)."""

import os
import sys

import numpy as np
import pytest

import parity_cases as pc
from conftest import assert_normwise, assert_stats, load_json, load_npz, to_np
from oracle.cvmatrix_oracle import (
    OracleCVMatrix,
    OraclePartitioner,
    benchmark_inputs,
    complement_indices,
    naive_training_matrices,
)

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module", params=["lazy_fit", "eager_fit"])
def amd(hip_device, request):
    """Every test runs twice: with the package defaults (fit() lazy: a batched call over folds that
    partition the rows is served by one sweep; private device copies padded to 16-byte rows, so
    every shape takes the LDS-DMA kernels) and with CVM_LAZY_FIT=0 CVM_PAD=0 (fit kernel, then the
    fold update kernels; the caller's shapes as they are: unaligned ones take the general kernels),
    so both routes and both kernel families see all the cases."""
    import os

    import cvmatrix_amd

    from cvmatrix_amd import _lib

    _lib.load()  # fails loudly if the extension is missing
    old = {k: os.environ.get(k) for k in ("CVM_LAZY_FIT", "CVM_PAD")}
    os.environ["CVM_LAZY_FIT"] = "1" if request.param == "lazy_fit" else "0"
    os.environ["CVM_PAD"] = "1" if request.param == "lazy_fit" else "0"
    yield cvmatrix_amd
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def make_factory(amd):
    def make(flags, ddof, dtype=np.float64):
        return amd.CVMatrix(*flags, ddof=ddof, dtype=dtype)

    return make


# ---------------------------------------------------------------- golden vectors (G1-G7)
def test_g1_inline_fixtures(amd):
    pc.run_g1(make_factory(amd), amd.Partitioner, TOL)


def test_g2_readme_quickstart(amd):
    pc.run_g2(make_factory(amd), amd.Partitioner, TOL)


@pytest.mark.parametrize("name", pc.g3_cases())
def test_g3_flag_sweep(amd, name):
    pc.run_g3_case(name, make_factory(amd), amd.Partitioner, TOL)


@pytest.mark.parametrize("chunk", range(8))
def test_g3_leave_one_out_sweep(amd, chunk):
    """The reference's whole leave-one-out sweep (tests/test_cvmatrix.py:1357-1396: 16 flag sets x
    weights x ddof x Y/None, first 20 folds) against its golden outputs: one call per fold (the
    reference's loop, indices inside the kernel arguments) and all 20 folds in one batched call."""
    cases = pc.g3loo_cases()
    assert len(cases) == 128
    for name in cases[chunk::8]:
        pc.run_g3loo_case(name, make_factory(amd), TOL)
        pc.run_g3loo_case(name, make_factory(amd), TOL, batched=True)


# BASELINE.md section 4 for float32: "error must not exceed 2x NumPy-fp32's own error".  The only
# allowance on top is EIGHT float32 roundings of the scale (9.5e-7): result and yardstick are both
# float32 arrays, and where the yardstick itself is one or two roundings (uncentred sums, where
# NumPy's blocked sgemm happens to be exact to a rounding) "twice" is below the resolution of the
# comparison.  Calibration (round 3, CVM_FP32_REPORT): over the 1904 float32 comparisons of this
# file 18 exceed twice the yardstick, by at most 0.6 roundings; of the 300 + 500 randomised cases
# (tools/fuzz_all.py, fuzz_small.py) the first to fail a ONE-rounding allowance exceeded it by 1.1
# (error 4.1 roundings against a yardstick of 1.0); a later run of 1500 + 1500 + 800 cases with other
# seeds found one 4.0 roundings over twice its yardstick (error 8.7 roundings, yardstick 2.4: the
# unweighted, uncentred XTY of a 6000-row fold at K=640, M=70 -- the MFMA accumulates a row split in
# float32 where OpenBLAS blocks its sums), so the allowance is eight.  The 2e-5 / 2e-6 floors of
# rounds 1-2 were never needed.
from cvmatrix_amd.fp32_gate import FP32_EPS, fp32_floor  # noqa: E402  (the gate's one definition: cvmatrix_amd/fp32_gate.py)
# Round 4: the float32 Gram kernels fold their accumulators into a second set every 1024 rows (FOLD_STAGES * 16; two-level
# sums, like the blocked sgemm of the reference's BLAS), whatever the row-split plan: the allowance on top
# of twice the yardstick is back to two roundings (result and yardstick are both float32 arrays: where the
# yardstick is itself one rounding, "twice" is below the resolution of the comparison).
# float32 statistics against the float64 oracle on the same float32 inputs: the product sums in
# float64 and rounds once, so means agree to a rounding; a standard deviation is the root of a
# difference of sums and may lose a few more
F32_STAT_RTOL = 2e-6
FP32_FLOOR = fp32_floor()      # two roundings; one more per extra partial under a forced split plan (fp32_gate.py)


def assert_fp32_like_reference(got, ref64, ref32, what, floor=FP32_FLOOR):
    """BASELINE.md section 4 for float32: the error against the float64 reference is at most
    twice the error of the reference's own float32 arithmetic (`ref32`: the oracle run in
    float32 on the same float32 inputs), plus two float32 roundings of the scale."""
    got = to_np(got).astype(np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    ref32 = np.asarray(ref32, dtype=np.float64)
    scale = max(np.abs(ref64).max(), np.finfo(np.float64).tiny)
    err = np.abs(got - ref64).max() / scale
    yard = np.abs(ref32 - ref64).max() / scale
    if os.environ.get("CVM_FP32_REPORT"):         # (calibration runs: every comparison's two errors)
        with open(os.environ["CVM_FP32_REPORT"], "a") as fh:
            fh.write(f"{what}\t{err:.3e}\t{yard:.3e}\t{floor:.1e}\n")
    assert err <= 2 * yard + floor, f"{what}: error {err:.3e} > 2 x reference float32 error {yard:.3e} + {floor}"


@pytest.mark.parametrize("K,weighted,dtype", [(70, True, np.float64), (70, False, np.float64), (500, True, np.float64),
                                              (500, True, np.float32), (200, False, np.float32)])
def test_leave_one_out_flag_sweep_rows_kernel(amd, K, weighted, dtype):
    """Every flag combination x ddof x Y/None on the route the reference's published
    leave-one-out benchmark takes (small_rows_kernel: one-row folds, rows that are not whole
    128-byte lines), against the oracle (which test_oracle_golden.py pins to the reference on
    the same 128 configurations at K = 8).  float32: against the float64 oracle with the
    oracle's own float32 run as the yardstick."""
    import itertools

    rng = np.random.default_rng(1000 + K)
    N, M = 90, 3
    X = (rng.random((N, K)) * 2.0 + rng.random((1, K))).astype(dtype)
    Y = (rng.standard_normal((N, M)) + 1.0).astype(dtype)
    w = (rng.random(N) + 0.05).astype(dtype)
    w[rng.choice(N, size=9, replace=False)] = 0.0
    folds = [np.array([f]) for f in range(24)]
    f32 = dtype is np.float32
    X64, Y64, w64 = X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64)
    for flags in itertools.product([False, True], repeat=4):
        for ddof in (0, 1):
            for hasY in (True, False):
                m = amd.CVMatrix(*flags, ddof=ddof, dtype=dtype)
                o = OracleCVMatrix(*flags, ddof=ddof)
                m.fit(X, Y if hasY else None, w if weighted else None)
                o.fit(X64, Y64 if hasY else None, w64 if weighted else None)
                if f32:
                    o32 = OracleCVMatrix(*flags, ddof=ddof, dtype=np.float32)
                    o32.fit(X, Y if hasY else None, w if weighted else None)
                what = f"K={K} flags={flags} ddof={ddof} Y={hasY}"
                if hasY:
                    (bx, by), bst = m.training_XTX_XTY_batched(folds)
                else:
                    bx, bst = m.training_XTX_batched(folds)
                for f in (0, 7, 23):
                    if hasY:
                        (rx, ry), rst = o.training_XTX_XTY(folds[f])
                        if f32:
                            (sx, sy), _ = o32.training_XTX_XTY(folds[f])
                            assert_fp32_like_reference(by[f], ry, sy, what + " XTY")
                        else:
                            assert_normwise(by[f], ry, TOL, what + " XTY")
                    else:
                        rx, rst = o.training_XTX(folds[f])
                        if f32:
                            sx, _ = o32.training_XTX(folds[f])
                    if f32:
                        assert_fp32_like_reference(bx[f], rx, sx, what + " XTX")
                        for a_, b_ in zip(tuple(None if s is None else s[f] for s in bst), rst):
                            assert (a_ is None) == (b_ is None)
                            if b_ is not None:
                                np.testing.assert_allclose(to_np(a_).astype(np.float64), b_, rtol=F32_STAT_RTOL)
                    else:
                        assert_normwise(bx[f], rx, TOL, what + " XTX")
                        assert_stats(tuple(None if s is None else s[f] for s in bst), rst, TOL, what)


def test_g4_example_zero_weight_and_str_label(amd):
    pc.run_g4(make_factory(amd), amd.Partitioner, TOL)


def test_g5_error_messages(amd):
    pc.run_g5(amd.CVMatrix, amd.Partitioner)


def test_g7_none_pattern(amd):
    pc.run_g7(amd.CVMatrix)


# ---------------------------------------------------------------- digests at full shapes
@pytest.mark.parametrize("name", ["c2", "c3", "c4s"])
def test_g6_digest_fp64(amd, name):
    z = load_npz("g6_digest.npz")
    meta = load_json("g6_digest_meta.json")[name]
    X, Y, w, folds = benchmark_inputs(meta["N"], meta["K"], meta["M"], meta["P"])
    m = amd.CVMatrix(*meta["flags"], ddof=1)
    m.fit(X, Y, w if meta["weighted"] else None)
    p = amd.Partitioner(folds)
    labels = [int(f) for f in z[f"{name}/fold_labels"]]
    # single-fold calls
    for f in labels[:2]:
        (xtx, xty), st = m.training_XTX_XTY(p.get_validation_indices(f))
        pc.check_digest(z, name, f, xtx, xty, st, TOL)
    # one batched call over all folds
    (bx, by), bst = m.training_XTX_XTY_batched(p)
    keys = list(p.folds_dict)
    for f in labels:
        i = keys.index(f)
        st = tuple(None if s is None else s[i] for s in bst)
        pc.check_digest(z, name, f, bx[i], by[i], st, TOL)
    # the result is exactly symmetric (the kernel mirrors the upper triangle)
    assert bool((bx[0] == bx[0].T).all())


def test_g6_digest_fp32_c5_scaled(amd):
    """C5 shape (K=4096, M=1, fp32), N scaled to 8000: fp32 result vs the fp64 reference
    must be no worse than 2x the reference's own fp32 error (+ two float32 roundings of the scale)."""
    name = "c5s"
    z = load_npz("g6_digest.npz")
    meta = load_json("g6_digest_meta.json")[name]
    X, Y, w, folds = benchmark_inputs(meta["N"], meta["K"], meta["M"], meta["P"],
                                      dtype=np.float32)
    m = amd.CVMatrix(dtype=np.float32)
    m.fit(X, Y, w)
    p = amd.Partitioner(folds)
    (bx, by), bst = m.training_XTX_XTY_batched(p)
    assert bx.dtype.is_floating_point and bx.element_size() == 4
    keys = list(p.folds_dict)
    sx, sy = z[f"{name}/samp_x"], z[f"{name}/samp_y"]
    for f in [int(f) for f in z[f"{name}/fold_labels"]]:
        i = keys.index(f)
        k = f"{name}/fold{f}"
        x64 = to_np(bx[i]).astype(np.float64)
        y64 = to_np(by[i]).astype(np.float64)
        bound_x = 2 * float(z[f"{k}/ref32_XTX_relfro"]) + FP32_FLOOR
        bound_y = 2 * float(z[f"{k}/ref32_XTY_relfro"]) + FP32_FLOOR
        # sampled entries everywhere; whole rows of XTX and the whole XTY where the fixtures hold
        # them (folds 0 and 19): the norm of the difference against BASELINE.md section 4's bound,
        # twice NumPy's own float32 error -- no extra slack
        ex = np.abs(x64[sx[:, 0], sx[:, 1]] - z[f"{k}/XTX_samp"]).max() / z[f"{k}/XTX_max"]
        ey = np.abs(y64[sy[:, 0], sy[:, 1]] - z[f"{k}/XTY_samp"]).max() / z[f"{k}/XTY_max"]
        assert ex <= bound_x and ey <= bound_y, (f, ex, ey, bound_x, bound_y)
        pc.check_strips(name, f, x64, y64, min(bound_x, bound_y))
        assert abs(np.linalg.norm(x64) - z[f"{k}/XTX_fro"]) <= bound_x * z[f"{k}/XTX_fro"]
        assert abs(np.linalg.norm(y64) - z[f"{k}/XTY_fro"]) <= bound_y * z[f"{k}/XTY_fro"]
        for n_, g_ in zip(("muX", "sdX", "muY", "sdY"), bst):
            np.testing.assert_allclose(to_np(g_[i]), z[f"{k}/{n_}"], rtol=2e-5)


# ---------------------------------------------------------------- BASELINE shapes at FULL size
@pytest.mark.parametrize("wl", ["C4", "C5"])
def test_full_size_properties_c4_c5(amd, hip_device, wl):
    """C4 (N=1e6, K=1024, M=32, 64 folds, fp64) and C5 (N=2e5, K=4096, M=1, 20 folds, fp32) at
    their FULL sizes, inputs generated on the device (bench.py's generator), checked through
    size-independent properties:
      (i)   partition linearity with all flags off: sum_f (G - XTX_f) = G (and the same for XTY);
      (ii)  two folds with all flags on against a from-scratch float64 computation of the centred
            and scaled training-set matrices (bench.direct_fold_check: library GEMMs, the naive
            definition) -- 1e-10 norm-wise for fp64, twice NumPy's float32 error for fp32;
      (iii) exact symmetry of every XTX, and a bitwise identical repeat."""
    import torch

    import bench

    N, K, M, P, weighted, flags, npdt = bench.WORKLOADS[wl]
    tdt = torch.float64 if npdt is np.float64 else torch.float32
    dev = hip_device
    Xd, Yd, wd = bench.synth_device_rows(torch, dev, torch.arange(N, device=dev), N, K, M, tdt, 42)
    labels = torch.arange(N, device=dev) % P
    # (i) linearity, flags off
    m0 = amd.CVMatrix(False, False, False, False, dtype=npdt, copy=False)
    m0.fit(Xd, Yd, wd)
    batch = m0.prepare_folds_from_labels(labels, P)
    (bx, by), _ = m0.training_XTX_XTY_batched(batch)
    G, H = m0.XTX.double(), m0.XTY.double()
    lin_x = (P * G - bx.double().sum(0) - G).abs().max() / G.abs().max()
    lin_y = (P * H - by.double().sum(0) - H).abs().max() / H.abs().max()
    lin_tol = 1e-11 if npdt is np.float64 else 5e-6   # (20 float32 roundings of magnitude |G|)
    assert float(lin_x) <= lin_tol and float(lin_y) <= lin_tol, (float(lin_x), float(lin_y))
    del bx, by, m0
    torch.cuda.empty_cache()
    # (ii) + (iii), all flags on
    m = amd.CVMatrix(*flags, ddof=1, dtype=npdt, copy=False)
    m.fit(Xd, Yd, wd)
    batch = m.prepare_folds_from_labels(labels, P)
    (bx, by), st = m.training_XTX_XTY_batched(batch)
    assert bool((bx == bx.transpose(1, 2)).all())
    for f in (0, P - 1):
        val = torch.nonzero(labels == batch.labels[f]).reshape(-1)
        got = (bx[f], by[f], st[0][f], st[1][f])
        errs = bench.direct_fold_check(torch, None, 1, Xd, Yd, wd, val, 0, 0, 1, flags, got, dev,
                                       yardstick=npdt is np.float32)
        if npdt is np.float64:
            bx_, by_, bs_ = 1e-10, 1e-10, 1e-10
        else:
            # at most twice the error the reference's algorithm makes in
            # plain float32 on the same problem (bench.fp32_algorithm_error), no other slack
            bx_, by_, bs_ = 2 * errs[4], 2 * errs[5], 1e-6
        assert errs[0] <= bx_ and errs[1] <= by_, (wl, f, errs)
        assert errs[2] <= bs_ and errs[3] <= bs_, (wl, f, errs)
    (cx, cy), _ = m.training_XTX_XTY_batched(batch)
    assert torch.equal(cx, bx) and torch.equal(cy, by)


# ---------------------------------------------------------------- oracle on seeded inputs
def _compare_with_oracle(amd, X, Y, w, fold_lists, flags, ddof=1, tol=TOL, dtype=np.float64):
    m = amd.CVMatrix(*flags, ddof=ddof, dtype=dtype)
    o = OracleCVMatrix(*flags, ddof=ddof)
    m.fit(X, Y, w)
    o.fit(X, Y, w)
    if Y is not None:
        (bx, by), bst = m.training_XTX_XTY_batched(fold_lists)
    else:
        bx, bst = m.training_XTX_batched(fold_lists)
        by = None
    for i, v in enumerate(fold_lists):
        if Y is not None:
            (rx, ry), rst = o.training_XTX_XTY(np.asarray(v))
            assert_normwise(by[i], ry, tol, f"fold{i} XTY")
        else:
            rx, rst = o.training_XTX(np.asarray(v))
        assert_normwise(bx[i], rx, tol, f"fold{i} XTX")
        assert_stats(tuple(None if s is None else s[i] for s in bst), rst, tol, f"fold{i}")
    return m, o


@pytest.mark.parametrize("K,M", [(1, 1), (7, 3), (129, 33), (130, 16), (257, 70), (384, 0)])
def test_shapes_ragged_empty_and_unaligned(amd, K, M):
    """Odd K (unaligned row starts -> scalar-load variant), K/M just past a tile edge,
    M > 32 (several Y chunks), Y absent; ragged folds incl. an empty one and one with a
    single row; all against the oracle."""
    rng = np.random.default_rng(100 + K)
    N = 700
    X = rng.standard_normal((N, K)) + 0.5
    Y = rng.random((N, M)) if M else None
    w = rng.random(N)
    w[rng.choice(N, 50, replace=False)] = 0
    perm = rng.permutation(N)
    folds = [perm[:300], perm[300:301], np.zeros(0, dtype=int), perm[301:650], perm[650:]]
    for flags in [(True,) * 4, (False,) * 4, (True, False, True, False)]:
        _compare_with_oracle(amd, X, Y, w, folds, flags)
    _compare_with_oracle(amd, X, Y, None, folds, (True,) * 4)


def test_duplicates_and_negative_indices(amd):
    """NumPy fancy-index semantics: duplicates count twice, negatives wrap."""
    rng = np.random.default_rng(5)
    X, Y, w = rng.random((50, 6)), rng.random((50, 2)), rng.random(50)
    v = np.array([3, 3, -1, 10, -50])
    _compare_with_oracle(amd, X, Y, w, [v], (True,) * 4)
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    with pytest.raises(IndexError):
        m.training_XTX(np.array([50]))


def test_one_dimensional_inputs_and_y_none(amd):
    """tests/test_cvmatrix.py:1083-1145."""
    X = np.array([1, 2, 3, 4, 5])
    Y = np.array([5, 4, 3, 2, 1])
    w = np.array([2, 4, 6, 8, 10])
    m, _ = _compare_with_oracle(amd, X, Y, w, [np.array([0, 1]), np.array([4])], (True,) * 4)
    assert m.X.shape == (5, 1) and m.Y.shape == (5, 1)
    xtx, st = m.training_XTX(np.array([2, 3]))
    assert xtx.shape == (1, 1) and st[0].shape == (1, 1) and st[2] is None
    _compare_with_oracle(amd, X, None, w, [np.array([0, 1])], (True,) * 4)


def test_constant_column_is_exact(amd):
    """A constant-one column must get variance exactly 0 -> std replaced by 1
    (cvmatrix.py:1128), also WITH weights: the kernel reduces w, w*x and w*x*x in the same
    order (SURVEY 7 'hard parts' 4; the reference itself only guarantees this unweighted,
    tests/test_cvmatrix.py:1045-1081)."""
    rng = np.random.default_rng(11)
    N, K = 5000, 40
    X = rng.random((N, K))
    X[:, 7] = 1.0
    Y = rng.random((N, 3))
    Y[:, 1] = 1.0
    w = rng.random(N)
    folds = [np.arange(i, N, 7) for i in range(7)]
    for weights in (None, w):
        m = amd.CVMatrix()
        m.fit(X, Y, weights)
        (_, _), (muX, sdX, muY, sdY) = m.training_XTX_XTY_batched(folds)
        assert bool((sdX[:, 0, 7] == 1.0).all()) and bool((sdY[:, 0, 1] == 1.0).all())
        assert bool((muX[:, 0, 7] == 1.0).all())


def test_ones_weights_equal_unweighted(amd):
    """tests/test_cvmatrix.py:978-1018."""
    rng = np.random.default_rng(3)
    X, Y = rng.random((400, 20)), rng.random((400, 4))
    folds = [np.arange(i, 400, 4) for i in range(4)]
    a = amd.CVMatrix()
    a.fit(X, Y, np.ones(400))
    b = amd.CVMatrix()
    b.fit(X, Y, None)
    (ax, ay), ast = a.training_XTX_XTY_batched(folds)
    (bx, by), bst = b.training_XTX_XTY_batched(folds)
    assert_normwise(ax, to_np(bx), 1e-13)
    assert_normwise(ay, to_np(by), 1e-13)
    for s, t in zip(ast, bst):
        np.testing.assert_allclose(to_np(s), to_np(t), rtol=1e-13)


def test_refit_switches_matrices(amd):
    """tests/test_cvmatrix.py:1020-1043: fit again with X and Y swapped."""
    rng = np.random.default_rng(9)
    X, Y, w = rng.random((300, 5)), rng.random((300, 9)), rng.random(300)
    folds = [np.arange(0, 100), np.arange(100, 300)]
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    m.training_XTX_XTY_batched(folds)
    m.fit(Y, X, None)
    o = OracleCVMatrix()
    o.fit(Y, X, None)
    (bx, by), _ = m.training_XTX_XTY_batched(folds)
    for i, v in enumerate(folds):
        (rx, ry), _ = o.training_XTX_XTY(v)
        assert_normwise(bx[i], rx, TOL)
        assert_normwise(by[i], ry, TOL)


def test_dtype_preserved_and_copy_semantics(amd, hip_device):
    """tests/test_cvmatrix.py:1147-1250 on the device: outputs carry the constructor dtype;
    copy=False aliases a matching device tensor, copy=True does not."""
    import torch

    rng = np.random.default_rng(2)
    X = rng.random((64, 4))
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        m = amd.CVMatrix(dtype=dt)
        m.fit(X, X[:, :2], np.ones(64))
        (xtx, xty), st = m.training_XTX_XTY(np.arange(8))
        assert xtx.dtype == tdt and xty.dtype == tdt and all(s.dtype == tdt for s in st)
    Xd = torch.from_numpy(X).to(hip_device)
    m = amd.CVMatrix(copy=False)
    m.fit(Xd)
    assert m.X.data_ptr() == Xd.data_ptr()
    m = amd.CVMatrix(copy=True)
    m.fit(Xd)
    assert m.X.data_ptr() != Xd.data_ptr()
    with pytest.raises(TypeError):
        amd.CVMatrix(dtype=np.int32)
    with pytest.raises(ValueError, match="Invalid backend"):
        amd.CVMatrix(backend="tpu")


def test_deterministic_and_batch_invariant(amd):
    """Fixed-order reductions: the same call twice is bit-identical; a fold computed alone
    or inside a batch agrees to rounding (the row split differs)."""
    rng = np.random.default_rng(21)
    X, Y, w = rng.random((20000, 256)), rng.random((20000, 8)), rng.random(20000)
    folds = [np.arange(i, 20000, 5) for i in range(5)]
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    g1 = m.XTX.clone()
    (a, b), sa = m.training_XTX_XTY_batched(folds)
    (c, d), sc = m.training_XTX_XTY_batched(folds)
    assert bool((a == c).all()) and bool((b == d).all())
    assert all(bool((s == t).all()) for s, t in zip(sa, sc))
    m.fit(X, Y, w)
    assert bool((g1 == m.XTX).all())
    (e, f), _ = m.training_XTX_XTY(folds[2])
    assert_normwise(e, to_np(a[2]), 1e-12)
    assert_normwise(f, to_np(b[2]), 1e-12)


def test_small_workspace_walks_folds_in_batches(amd):
    """cvm_fold_update with a workspace that holds only part of the folds."""
    rng = np.random.default_rng(8)
    X, Y, w = rng.random((3000, 140)), rng.random((3000, 4)), rng.random(3000)
    folds = [np.arange(i, 3000, 12) for i in range(12)]
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    (a, b), _ = m.training_XTX_XTY_batched(folds)
    import torch

    from cvmatrix_amd import _lib

    lib = _lib.load()
    full = lib.cvm_fold_workspace_bytes(12, 3000, 250, 140, 4, _lib.CVM_F64, 0x3F)
    m._ws = torch.empty(full // 5, dtype=torch.uint8, device=m.device)
    m._workspace = lambda n: m._ws  # keep the undersized workspace
    (c, d), _ = m.training_XTX_XTY_batched(folds)
    assert_normwise(c, to_np(a), 1e-12)
    assert_normwise(d, to_np(b), 1e-12)


# ---------------------------------------------------------------- properties at full size
def test_full_size_partition_linearity_c2(amd):
    """C2 (N=1e5,K=512,M=16,P=10, no weights, no preprocessing): the folds partition the
    rows, so sum_f (G - G_train_f) = G and sum_f (H - H_train_f) = H."""
    X, Y, w, folds = benchmark_inputs(100000, 512, 16, 10)
    m = amd.CVMatrix(False, False, False, False)
    m.fit(X, Y, None)
    p = amd.Partitioner(folds)
    (bx, by), st = m.training_XTX_XTY_batched(p)
    assert st == (None, None, None, None)
    G, H = m.XTX.double(), m.XTY.double()
    sx = (G[None] - bx.double()).sum(0)
    sy = (H[None] - by.double()).sum(0)
    assert_normwise(sx, to_np(G), 1e-12, "sum of validation Grams")
    assert_normwise(sy, to_np(H), 1e-12)
    # and the fit-stage Gram itself against a float64 matmul on the device
    import torch

    Xd = m.X
    assert_normwise(G, to_np(Xd.T @ Xd), 1e-12, "fit Gram")
    assert_normwise(H, to_np(Xd.T @ m.Y), 1e-12, "fit XTY")


def test_full_size_c3_naive_crosscheck_one_fold(amd):
    """C3: one fold against the direct training-set computation (the reference's own
    equivalence test, tests/test_cvmatrix.py:420-537, atol 1e-8) -- independent of the
    subtract-and-correct algebra."""
    X, Y, w, folds = benchmark_inputs(100000, 512, 16, 10)
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    p = amd.Partitioner(folds)
    (xtx, xty), st = m.training_XTX_XTY(p.get_validation_indices(3))
    op = OraclePartitioner(folds)
    (nx, ny), nst = naive_training_matrices(X, Y, w, complement_indices(op, 3),
                                            True, True, True, True, 1)
    np.testing.assert_allclose(to_np(xtx), nx, atol=1e-8, rtol=1e-7)
    np.testing.assert_allclose(to_np(xty), ny, atol=1e-8, rtol=1e-7)
    assert_stats(st, nst, 1e-9, "c3 naive")


def test_fallback_kernel_matches_fast_kernel(amd):
    """float64 problems normally run the 4+4-wave LDS-DMA kernel; CVM_FORCE_FALLBACK=1 (read
    once per process) sends them through the general register-staged kernel that float32,
    odd K and odd M use.  Run the same problem in a child process with the switch set and
    compare with this process's result and with the oracle."""
    import os
    import subprocess
    import sys
    import tempfile

    rng = np.random.default_rng(77)
    N, K, M = 6000, 256, 6
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    folds = [np.arange(i, N, 4) for i in range(4)]
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    (ax, ay), ast = m.training_XTX_XTY_batched(folds)
    with tempfile.TemporaryDirectory() as td:
        np.savez(os.path.join(td, "in.npz"), X=X, Y=Y, w=w)
        code = (
            "import numpy as np, sys\n"
            f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
            "from cvmatrix_amd import CVMatrix\n"
            f"z = np.load({os.path.join(td, 'in.npz')!r})\n"
            "m = CVMatrix(); m.fit(z['X'], z['Y'], z['w'])\n"
            "N = z['X'].shape[0]\n"
            "(x, y), st = m.training_XTX_XTY_batched([np.arange(i, N, 4) for i in range(4)])\n"
            f"np.savez({os.path.join(td, 'out.npz')!r}, x=x.cpu().numpy(), y=y.cpu().numpy(),\n"
            "         g=m.XTX.cpu().numpy(), mu=st[0].cpu().numpy(), sd=st[1].cpu().numpy())\n"
        )
        env = dict(os.environ, CVM_FORCE_FALLBACK="1")
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
        z = np.load(os.path.join(td, "out.npz"))
    assert_normwise(ax, z["x"], 1e-12, "fallback vs fast XTX")
    assert_normwise(ay, z["y"], 1e-12, "fallback vs fast XTY")
    assert_normwise(m.XTX, z["g"], 1e-12, "fallback vs fast fit Gram")
    np.testing.assert_allclose(to_np(ast[0]), z["mu"], rtol=1e-12)
    np.testing.assert_allclose(to_np(ast[1]), z["sd"], rtol=1e-12)
    o = OracleCVMatrix()
    o.fit(X, Y, w)
    (rx, ry), _ = o.training_XTX_XTY(folds[1])
    assert_normwise(z["x"][1], rx, TOL)
    assert_normwise(z["y"][1], ry, TOL)


def test_one_sweep_fit_matches_two_stage(amd):
    """fit(folds=partition) forms the full-data matrices as the sum of the folds' validation
    matrices (cvm_sweep_fit) and the batched update reuses the partials (cvm_sweep_folds):
    same results as fit() + training_XTX_XTY_batched() to rounding, and as the oracle."""
    rng = np.random.default_rng(31)
    N, K, M, P = 9000, 384, 10, 7
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    w[rng.choice(N, 500, replace=False)] = 0
    part = amd.Partitioner(rng.integers(0, P, size=N))       # ragged folds
    for weights in (w, None):
        a = amd.CVMatrix()
        a.fit(X, Y, weights)
        (ax, ay), ast = a.training_XTX_XTY_batched(part)
        b = amd.CVMatrix()
        b.fit(X, Y, weights, folds=part)
        assert b.sweep_folds is not None and b.sweep_folds.is_partition
        assert_normwise(b.XTX, to_np(a.XTX), 1e-12, "sweep fit G")
        assert_normwise(b.XTY, to_np(a.XTY), 1e-12, "sweep fit H")
        np.testing.assert_allclose(to_np(b.sum_X), to_np(a.sum_X), rtol=1e-12)
        (bx, by), bst = b.training_XTX_XTY_batched(b.sweep_folds)
        assert_normwise(bx, to_np(ax), 1e-11, "sweep XTX")
        assert_normwise(by, to_np(ay), 1e-11, "sweep XTY")
        for s, t in zip(ast, bst):
            np.testing.assert_allclose(to_np(t), to_np(s), rtol=1e-11)
        # other methods on the sweep batch, and a different fold set (normal path) still work
        cx, cst = b.training_XTX_batched(b.sweep_folds)
        assert_normwise(cx, to_np(ax), 1e-11)
        st = b.training_statistics_batched(b.sweep_folds)
        np.testing.assert_allclose(to_np(st[1]), to_np(ast[1]), rtol=1e-11)
        o = OracleCVMatrix()
        o.fit(X, Y, weights)
        keys = list(part.folds_dict)
        (rx, ry), rst = o.training_XTX_XTY(part.get_validation_indices(keys[2]))
        assert_normwise(bx[2], rx, TOL)
        assert_normwise(by[2], ry, TOL)
        assert_stats(tuple(s[2] for s in bst), rst, TOL)
        (dx, dy), _ = b.training_XTX_XTY(part.get_validation_indices(keys[3]))
        assert_normwise(dx, to_np(ax[3]), 1e-11)
    with pytest.raises(ValueError, match="exactly once"):
        amd.CVMatrix().fit(X, Y, w, folds=[np.arange(10), np.arange(5, N)])


def test_one_sweep_digest_c3(amd):
    """The one-sweep path at the full C3 shape against the reference digests."""
    z = load_npz("g6_digest.npz")
    X, Y, w, folds = benchmark_inputs(100000, 512, 16, 10)
    m = amd.CVMatrix()
    p = amd.Partitioner(folds)
    m.fit(X, Y, w, folds=p)
    (bx, by), bst = m.training_XTX_XTY_batched(m.sweep_folds)
    for f in (0, 3, 9):
        pc.check_digest(z, "c3", f, bx[f], by[f], tuple(s[f] for s in bst), TOL)


@pytest.mark.parametrize("K,M", [(1, 1), (7, 0), (66, 3), (129, 33), (257, 70)])
def test_small_fold_direct_path(amd, K, M):
    """Folds of at most 32 rows (leave-one-out and neighbours) take the direct, HBM-bound
    kernels (small_stats / small_apply) instead of the MFMA Gram + finalize sequence: ragged
    tiny folds incl. empty, 1-row and 32-row ones, odd K, tile edges, several flag sets,
    weighted and unweighted, against the oracle."""
    rng = np.random.default_rng(200 + K)
    N = 400
    X = rng.standard_normal((N, K)) + 0.5
    Y = rng.random((N, M)) if M else None
    w = rng.random(N)
    w[rng.choice(N, 40, replace=False)] = 0
    perm = rng.permutation(N)
    folds = [perm[0:1], perm[1:6], np.zeros(0, dtype=int), perm[6:38], perm[38:55], perm[55:56]]
    assert max(len(f) for f in folds) == 32
    for flags in [(True,) * 4, (False,) * 4, (False, True, True, False)]:
        _compare_with_oracle(amd, X, Y, w, folds, flags)
    _compare_with_oracle(amd, X, Y, None, folds, (True,) * 4, ddof=0)


def test_small_fold_loocv_fp32_and_constant_column(amd):
    """Leave-one-out in float32 against the float64 oracle, and the exact-variance property
    of a constant-one column on the direct path."""
    rng = np.random.default_rng(17)
    N, K, M = 300, 96, 4
    X = rng.random((N, K)).astype(np.float32)
    X[:, 5] = 1.0
    Y = rng.random((N, M)).astype(np.float32)
    w = rng.random(N).astype(np.float32)
    folds = [np.array([i]) for i in range(40)]
    m = amd.CVMatrix(dtype=np.float32)
    m.fit(X, Y, w)
    (bx, by), (muX, sdX, muY, sdY) = m.training_XTX_XTY_batched(folds)
    assert bool((sdX[:, 0, 5] == 1.0).all())
    o = OracleCVMatrix()
    o.fit(X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64))
    for i in (0, 7, 39):
        (rx, ry), rst = o.training_XTX_XTY(folds[i])
        rx[5, :] = rx[:, 5] = 0  # the clamped column: oracle divides by ~1e-8 there
        gx = to_np(bx[i]).astype(np.float64)
        gx[5, :] = gx[:, 5] = 0
        assert np.abs(gx - rx).max() <= 5e-4 * np.abs(rx).max()
        mask = np.ones(K, bool); mask[5] = False
        assert np.abs(to_np(by[i]).astype(np.float64)[mask] - ry[mask]).max() <= 5e-4 * np.abs(ry[mask]).max()
        np.testing.assert_allclose(to_np(muX[i]), rst[0], rtol=1e-5)


def test_race_screen_bitwise_repeatability_c3(amd):
    """The fast kernel hands LDS buffers from loader waves to compute waves behind a counted
    vmcnt and one barrier per stage; a misplaced wait would show up as rare wrong tiles.
    Screen: 25 back-to-back runs of fit + batched update (and the one-sweep path) at the C3
    shape must be bit-identical."""
    import torch

    X, Y, w, folds = benchmark_inputs(100000, 512, 16, 10)
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    b = m.prepare_folds(amd.Partitioner(folds))
    (x0, y0), s0 = m.training_XTX_XTY_batched(b)
    g0 = m.XTX.clone()
    Xd, Yd, wd = m.X, m.Y, m.weights.reshape(-1)
    for _ in range(25):
        m.fit(Xd, Yd, wd)
        (x1, y1), s1 = m.training_XTX_XTY_batched(b)
        assert torch.equal(g0, m.XTX) and torch.equal(x0, x1) and torch.equal(y0, y1)
        assert all(torch.equal(p, q) for p, q in zip(s0, s1))
    m.fit(Xd, Yd, wd, folds=b)
    (xs, ys), _ = m.training_XTX_XTY_batched(b)
    for _ in range(10):
        m.fit(Xd, Yd, wd, folds=b)
        (x1, y1), _ = m.training_XTX_XTY_batched(b)
        assert torch.equal(xs, x1) and torch.equal(ys, y1)


# ---------------------------------------------------------------- statistics-only path
@pytest.mark.parametrize("K,M,dtype", [(130, 16, np.float64), (129, 3, np.float64),
                                       (1100, 0, np.float64), (70, 5, np.float32),
                                       (1028, 300, np.float32)])
def test_training_statistics_streaming_kernel(amd, K, M, dtype):
    """training_statistics (cvmatrix.py:519-574) on folds of more than 32 rows runs the
    column-statistics kernel instead of the Gram kernel: every flag combination that changes
    its output map, weighted and unweighted, aligned and unaligned rows, several column
    blocks, ragged folds with an empty one; against the oracle, and against the statistics
    the matrix methods return for the same folds."""
    rng = np.random.default_rng(K + M)
    N = 2500
    X = (rng.standard_normal((N, K)) + 0.5).astype(dtype)
    Y = rng.random((N, M)).astype(dtype) if M else None
    w = rng.random(N).astype(dtype)
    w[rng.choice(N, 100, replace=False)] = 0
    perm = rng.permutation(N)
    folds = [perm[:900], perm[900:933], np.zeros(0, dtype=int), perm[933:1500], perm[1500:]]
    tol = TOL if dtype == np.float64 else F32_STAT_RTOL
    for flags in [(True,) * 4, (True, False, False, False), (False, False, True, True),
                  (False, True, False, True)]:
        for weights in (w, None):
            m = amd.CVMatrix(*flags, ddof=1, dtype=dtype)
            o = OracleCVMatrix(*flags, ddof=1, dtype=np.float64)
            m.fit(X, Y, weights)
            o.fit(X.astype(np.float64), None if Y is None else Y.astype(np.float64),
                  None if weights is None else weights.astype(np.float64))
            st = m.training_statistics_batched(folds)
            for i, v in enumerate(folds):
                ref = o.training_statistics(v)
                got = tuple(None if s is None else s[i] for s in st)
                assert_stats(got, ref, tol, f"flags={flags} fold{i}")
            one = m.training_statistics(folds[3])
            assert_stats(one, o.training_statistics(folds[3]), tol, "single fold")
            if dtype == np.float64 and M:
                (_, _), mst = m.training_XTX_XTY_batched(folds)
                for a_, b_ in zip(st, mst):
                    if a_ is not None and b_ is not None:
                        np.testing.assert_allclose(to_np(a_), to_np(b_), rtol=1e-12, atol=1e-13)


def test_training_statistics_constant_column_and_determinism(amd):
    """The streaming kernel keeps the exactness property of the Gram kernels (constant-one
    column -> std exactly 1, also weighted) and is bitwise reproducible."""
    rng = np.random.default_rng(77)
    N, K = 6000, 96
    X = rng.random((N, K)); X[:, 5] = 1.0
    Y = rng.random((N, 4)); Y[:, 2] = 1.0
    w = rng.random(N)
    folds = [np.arange(i, N, 6) for i in range(6)]
    for weights in (None, w):
        m = amd.CVMatrix()
        m.fit(X, Y, weights)
        muX, sdX, muY, sdY = m.training_statistics_batched(folds)
        assert bool((sdX[:, 0, 5] == 1.0).all()) and bool((sdY[:, 0, 2] == 1.0).all())
        assert bool((muX[:, 0, 5] == 1.0).all()) and bool((muY[:, 0, 2] == 1.0).all())
        again = m.training_statistics_batched(folds)
        for a_, b_ in zip((muX, sdX, muY, sdY), again):
            assert bool((a_ == b_).all())


# ---------------------------------------------------------------- fused mid-size folds
def _midsize_folds(rng, N, P):
    """P ragged folds of 33..~3N/P rows plus an empty one; every fold has more than 32 rows
    or none, so the batch takes the MFMA path, and there are enough folds for one unit each."""
    perm = rng.permutation(N)
    cuts = np.sort(rng.choice(np.arange(1, N // 40), P - 1, replace=False)) * 40
    folds = [f for f in np.split(perm, cuts) if len(f) > 32][:P]
    folds.insert(3, np.zeros(0, dtype=int))
    return folds


@pytest.mark.parametrize("K,M", [(130, 16), (200, 0), (384, 34), (512, 2)])
def test_fused_single_split_epilogue_matches_oracle(amd, K, M):
    """Many folds of 33..~500 rows: one unit per fold, so the float64 Gram kernel finishes
    every fold in its own epilogue (statistics from the streaming kernel first, no partials,
    no apply kernel).  K and M off the tile edges, Y absent, weighted and unweighted, every
    flag family, ragged folds with an empty one; each return shape against the oracle."""
    rng = np.random.default_rng(K * 7 + M)
    N = 24000
    X = rng.standard_normal((N, K)) + 0.5
    Y = rng.random((N, M)) if M else None
    w = rng.random(N)
    w[rng.choice(N, 800, replace=False)] = 0
    folds = _midsize_folds(rng, N, 120)
    assert max(len(f) for f in folds) > 32
    check = [0, 3, 4, len(folds) // 2, len(folds) - 1]
    for flags in [(True,) * 4, (False,) * 4, (True, False, True, False), (False, True, False, True)]:
        for weights in (w, None):
            m = amd.CVMatrix(*flags, ddof=1)
            o = OracleCVMatrix(*flags, ddof=1)
            m.fit(X, Y, weights)
            o.fit(X, Y, weights)
            if M:
                (bx, by), bst = m.training_XTX_XTY_batched(folds)
                by2, bst2 = m.training_XTY_batched(folds)
            else:
                bx, bst = m.training_XTX_batched(folds)
            bx1, bst1 = m.training_XTX_batched(folds)
            for i in check:
                v = folds[i]
                if M:
                    (rx, ry), rst = o.training_XTX_XTY(v)
                    assert_normwise(by[i], ry, TOL, f"fold{i} XTY")
                    ry2, rst2 = o.training_XTY(v)
                    assert_normwise(by2[i], ry2, TOL, f"fold{i} XTY only")
                    assert_stats(tuple(None if s is None else s[i] for s in bst2), rst2, TOL, f"fold{i} XTY only")
                else:
                    rx, rst = o.training_XTX(v)
                assert_normwise(bx[i], rx, TOL, f"fold{i} XTX")
                assert_stats(tuple(None if s is None else s[i] for s in bst), rst, TOL, f"fold{i}")
                rx1, rst1 = o.training_XTX(v)
                assert_normwise(bx1[i], rx1, TOL, f"fold{i} XTX only")
                assert_stats(tuple(None if s is None else s[i] for s in bst1), rst1, TOL, f"fold{i} XTX only")
            # exactly symmetric outputs
            t = bx[check[1] + 1]
            assert bool((t == t.T).all())


@pytest.mark.parametrize("K,M", [(132, 16), (200, 0), (384, 33), (516, 1)])
def test_fused_single_split_epilogue_float32(amd, K, M):
    """The same route in float32 (the LDS-DMA kernel finishes every fold in its own epilogue, tiles
    of float accumulators in LDS): against the float64 oracle with the oracle's own float32 run as
    the yardstick, every flag family, weighted and unweighted, ragged folds with an empty one;
    exactly symmetric; the same bits with and without XTY."""
    rng = np.random.default_rng(K * 11 + M)
    N = 24000
    X = (rng.standard_normal((N, K)) + 0.5).astype(np.float32)
    Y = rng.random((N, M)).astype(np.float32) if M else None
    w = rng.random(N).astype(np.float32)
    w[rng.choice(N, 800, replace=False)] = 0
    folds = _midsize_folds(rng, N, 120)
    check = [0, 3, 4, len(folds) // 2, len(folds) - 1]
    X64, Y64, w64 = X.astype(np.float64), None if Y is None else Y.astype(np.float64), w.astype(np.float64)
    for flags in [(True,) * 4, (False,) * 4, (True, False, True, False)]:
        for weights, weights64 in ((w, w64), (None, None)):
            m = amd.CVMatrix(*flags, ddof=1, dtype=np.float32)
            o = OracleCVMatrix(*flags, ddof=1)
            o32 = OracleCVMatrix(*flags, ddof=1, dtype=np.float32)
            m.fit(X, Y, weights)
            o.fit(X64, Y64, weights64)
            o32.fit(X, Y, weights)
            if M:
                (bx, by), bst = m.training_XTX_XTY_batched(folds)
            else:
                bx, bst = m.training_XTX_batched(folds)
            bx1, _ = m.training_XTX_batched(folds)
            assert torch_equal(bx, bx1)
            for i in check:
                v = folds[i]
                if M:
                    (rx, ry), rst = o.training_XTX_XTY(v)
                    (sx, sy), _ = o32.training_XTX_XTY(v)
                    assert_fp32_like_reference(by[i], ry, sy, f"fold{i} XTY", floor=FP32_FLOOR)
                else:
                    rx, rst = o.training_XTX(v)
                    sx, _ = o32.training_XTX(v)
                assert_fp32_like_reference(bx[i], rx, sx, f"fold{i} XTX", floor=FP32_FLOOR)
                for a_, b_ in zip(bst, rst):
                    assert (a_ is None) == (b_ is None)
                    if b_ is not None:
                        np.testing.assert_allclose(to_np(a_[i]).astype(np.float64), b_, rtol=F32_STAT_RTOL, atol=1e-7)
            t = bx[check[1] + 1]
            assert bool((t == t.T).all())


def test_fused_epilogue_equals_two_stage_path(amd):
    """CVM_NO_FUSED=1 (read once per process) keeps the partials + apply_kernel route for the
    same problem: both routes must agree to rounding, bitwise-reproducibly within a route."""
    import os
    import subprocess
    import sys
    import tempfile

    rng = np.random.default_rng(5)
    N, K, M, P = 30000, 256, 6, 200
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    X[:, 3] = 1.0
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    folds = [np.arange(i, N, P) for i in range(P)]
    (ax, ay), ast = m.training_XTX_XTY_batched(folds)
    (bx, by), _ = m.training_XTX_XTY_batched(folds)
    assert bool((ax == bx).all()) and bool((ay == by).all())
    assert bool((ast[1][:, 0, 3] == 1.0).all())          # constant column: std exactly 1
    with tempfile.TemporaryDirectory() as td:
        np.savez(os.path.join(td, "in.npz"), X=X, Y=Y, w=w)
        code = (
            "import numpy as np, sys\n"
            f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
            "from cvmatrix_amd import CVMatrix\n"
            f"z = np.load({os.path.join(td, 'in.npz')!r})\n"
            "m = CVMatrix(); m.fit(z['X'], z['Y'], z['w'])\n"
            f"N, P = z['X'].shape[0], {P}\n"
            "(x, y), st = m.training_XTX_XTY_batched([np.arange(i, N, P) for i in range(P)])\n"
            f"np.savez({os.path.join(td, 'out.npz')!r}, x=x[::17].cpu().numpy(), y=y[::17].cpu().numpy(),\n"
            "         mu=st[0].cpu().numpy(), sd=st[1].cpu().numpy())\n"
        )
        env = dict(os.environ, CVM_NO_FUSED="1")
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
        z = np.load(os.path.join(td, "out.npz"))
    assert_normwise(ax[::17], z["x"], 1e-12, "fused vs two-stage XTX")
    assert_normwise(ay[::17], z["y"], 1e-12, "fused vs two-stage XTY")
    np.testing.assert_allclose(to_np(ast[0]), z["mu"], rtol=1e-12)
    np.testing.assert_allclose(to_np(ast[1]), z["sd"], rtol=1e-12)


def test_fused_route_with_small_workspace_and_many_folds(amd):
    """The fused route walks the folds in batches when the workspace holds only some of
    their statistics vectors; and a single call over 40 000 leave-one-out folds (more than
    one internal batch of the small-fold route) matches the oracle on sampled folds."""
    import os
    if os.environ.get("CVM_NO_FUSED") or os.environ.get("CVM_FORCE_FALLBACK"):
        pytest.skip("the small workspace of this test only suffices for the fused route")
    import torch

    rng = np.random.default_rng(18)
    N, K, M, P = 16000, 256, 4, 250
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    folds = [np.arange(i, N, P) for i in range(P)]          # 64 rows each: one unit per fold
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    (a, b), ast = m.training_XTX_XTY_batched(folds)
    m._ws = torch.empty(40 * 8192, dtype=torch.uint8, device=m.device)   # ~30 folds per batch
    m._workspace = lambda n: m._ws
    (c, d), cst = m.training_XTX_XTY_batched(folds)
    assert bool((a == c).all()) and bool((b == d).all())
    for s, t in zip(ast, cst):
        assert bool((s == t).all())
    o = OracleCVMatrix()
    o.fit(X, Y, w)
    for i in (0, 29, 30, 31, 249):
        (rx, ry), rst = o.training_XTX_XTY(folds[i])
        assert_normwise(c[i], rx, TOL, f"fold{i}")
        assert_normwise(d[i], ry, TOL, f"fold{i}")
        assert_stats(tuple(s[i] for s in cst), rst, TOL, f"fold{i}")

    N2, K2, M2 = 40000, 48, 2
    X2, Y2, w2 = rng.random((N2, K2)), rng.random((N2, M2)), rng.random(N2)
    m2 = amd.CVMatrix()
    m2.fit(X2, Y2, w2)
    (x2, y2), st2 = m2.training_XTX_XTY_batched([np.array([i]) for i in range(N2)])
    o2 = OracleCVMatrix()
    o2.fit(X2, Y2, w2)
    for i in (0, 32767, 32768, 39999):
        (rx, ry), rst = o2.training_XTX_XTY(np.array([i]))
        assert_normwise(x2[i], rx, TOL, f"loocv{i}")
        assert_normwise(y2[i], ry, TOL, f"loocv{i}")
        assert_stats(tuple(s[i] for s in st2), rst, TOL, f"loocv{i}")


# ---------------------------------------------------------------- randomized shape sweep
def _sweep_cases():
    rng = np.random.default_rng(20260101)
    cases = []
    Ks = [2, 16, 62, 64, 66, 126, 128, 130, 190, 256, 258, 320, 386, 514]
    Ms = [0, 2, 4, 14, 16, 18, 32, 34, 66]
    for i in range(36):
        K = int(rng.choice(Ks))
        M = int(rng.choice(Ms))
        route = ("small", "fused", "units")[i % 3]
        cases.append((i, K, M, route))
    return cases


@pytest.mark.parametrize("i,K,M,route", _sweep_cases())
def test_random_shape_sweep_float64_fast_path(amd, i, K, M, route):
    """Even K and M (the float64 LDS-DMA kernel and its balanced diagonal waves / fused
    epilogue) at panel, block and MFMA-tile edges, through the three fold-size routes
    (<= 32 rows; many folds of one unit each; a few large folds split into units), ragged
    folds, zero weights, a random flag set; three folds per case against the oracle."""
    rng = np.random.default_rng(1000 + i)
    flags = tuple(bool(b) for b in rng.integers(0, 2, size=4))
    if route == "small":
        N, sizes = 1500, rng.integers(1, 33, size=40)
    elif route == "fused":
        N, sizes = 12000, rng.integers(33, 160, size=110)
    else:
        N, sizes = 9000, rng.integers(600, 2500, size=4)
    X = rng.standard_normal((N, K)) + 0.3
    Y = rng.random((N, M)) if M else None
    w = rng.random(N)
    w[rng.choice(N, N // 20, replace=False)] = 0
    perm = rng.permutation(N)
    cuts = np.cumsum(sizes)
    folds = [perm[a:b] for a, b in zip(np.concatenate([[0], cuts[:-1]]), cuts)]
    weights = w if i % 4 else None
    m = amd.CVMatrix(*flags, ddof=int(i % 2))
    o = OracleCVMatrix(*flags, ddof=int(i % 2))
    m.fit(X, Y, weights)
    o.fit(X, Y, weights)
    assert_normwise(m.XTX, o.XTX, TOL, "fit XTX")
    if M:
        (bx, by), bst = m.training_XTX_XTY_batched(folds)
    else:
        bx, bst = m.training_XTX_batched(folds)
    for f in (0, len(folds) // 2, len(folds) - 1):
        if M:
            (rx, ry), rst = o.training_XTX_XTY(folds[f])
            assert_normwise(by[f], ry, TOL, f"fold{f} XTY")
        else:
            rx, rst = o.training_XTX(folds[f])
        assert_normwise(bx[f], rx, TOL, f"fold{f} XTX")
        assert_stats(tuple(None if s is None else s[f] for s in bst), rst, TOL, f"fold{f}")
        t = bx[f]
        assert bool((t == t.T).all()), "XTX must be exactly symmetric"


def test_c_abi_from_plain_c(amd, tmp_path):
    """examples/cabi_client.c: the library driven from plain C11 through include/cvmhip.h
    (HIP runtime allocations, no Python objects, no torch): fit stage + fold stage, checked in
    the program itself against a direct float64 computation from the training rows."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cabi_client")
    libdir = os.path.join(root, "cvmatrix_amd")
    cmd = ["gcc", "-std=c11", "-O2", os.path.join(root, "examples", "cabi_client.c"),
           "-I" + os.path.join(root, "include"), "-I/opt/rocm/include", "-L" + libdir, "-lcvmhip",
           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm",
           "-o", exe]
    subprocess.run(cmd, check=True, timeout=300, capture_output=True)
    out = subprocess.run([exe], check=False, timeout=300, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


@pytest.mark.parametrize("N,P", [(100000, 10), (100003, 64), (5000, 5000), (777, 1)])
def test_device_partitioner_strided_and_leave_one_out_by_formula(amd, N, P):
    """Labels arange(N) % P (the reference benchmark's folds, benchmarks/benchmark.py:232) and
    arange(N) (leave-one-out): laid out by formula, equal to the host Partitioner."""
    import torch

    rng = np.random.default_rng(N)
    X, w = rng.random((N, 8)), rng.random(N)
    w[::7] = 0
    m = amd.CVMatrix()
    m.fit(X, None, w)
    labels = np.arange(N) % P
    hb = m.prepare_folds(amd.Partitioner(labels))
    db = m.prepare_folds_from_labels(torch.from_numpy(labels).to(m.device))
    assert db.labels == list(range(P)) and np.array_equal(db.host_offsets, hb.host_offsets)
    assert bool((db.idx == hb.idx).all()) and bool((db.offsets == hb.offsets).all())
    assert np.array_equal(db.nz_val, hb.nz_val)


@pytest.mark.parametrize("N,L", [(50000, 37), (4096, 4096), (1000, 1), (70001, 300), (60000, 4097),
                                 (100000, 100000), (30000, 20000000)])
def test_device_partitioner_matches_host_partitioner(amd, N, L):
    """cvm_partition_labels (CVMatrix.prepare_folds_from_labels): the same folds, in the same
    first-seen order with ascending indices, as the host Partitioner builds from the labels
    (cvmatrix/partitioner.py:89-107) -- and the same fold update from either."""
    import torch

    rng = np.random.default_rng(N + L)
    labels = rng.permutation(N) if L == N else rng.integers(0, L, size=N)
    K, M = 24, 2
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    w[rng.choice(N, N // 10, replace=False)] = 0
    m = amd.CVMatrix()
    m.fit(X, Y, w)
    part = amd.Partitioner(labels)
    hb = m.prepare_folds(part)
    for src in (labels, torch.from_numpy(labels).to(m.device)):
        db = m.prepare_folds_from_labels(src, n_labels=L)
        assert db.labels == [int(k) for k in part.folds_dict]
        assert np.array_equal(db.host_offsets, hb.host_offsets)
        assert bool((db.idx == hb.idx).all()) and bool((db.offsets == hb.offsets).all())
        assert np.array_equal(db.nz_val, hb.nz_val)
    if 1 < L <= 300:
        (a, b), sa = m.training_XTX_XTY_batched(hb)
        (c, d), sc = m.training_XTX_XTY_batched(db)
        assert bool((a == c).all()) and bool((b == d).all())
    with pytest.raises(ValueError):
        bad = labels.copy()
        bad[3] = L
        m.prepare_folds_from_labels(bad, n_labels=L)


@pytest.mark.parametrize("kind", ["str", "float", "float_nan", "object"])
def test_device_partitioner_takes_any_hashable_label(amd, kind):
    """partitioner.py:101-107 groups labels of any hashable kind: strings, floats and mixed objects go
    through ``prepare_folds_from_labels`` too (factorised on the host in first-seen order, grouped on
    the device) and give the host Partitioner's folds, labels and order."""
    rng = np.random.default_rng(17)
    N, K = 5000, 12
    codes = rng.integers(0, 23, size=N)
    if kind == "str":
        labels = np.array([f"site-{c:02d}" for c in codes])
    elif kind == "float":
        labels = codes.astype(np.float64) * 0.5 - 3.25
    elif kind == "float_nan":
        # nan != nan: every NaN label is a fold of its own in the reference's dict (partitioner.py:101-107)
        labels = codes.astype(np.float64) * 0.5 - 3.25
        labels[[7, 1234, 4999]] = np.nan
    else:
        pool = [("a", 1), "b", 2.5, 7, None, frozenset({3})] + [f"k{i}" for i in range(17)]
        labels = [pool[c] for c in codes]
    m = amd.CVMatrix()
    m.fit(rng.random((N, K)), None, rng.random(N) + 0.1)
    part = amd.Partitioner(labels)
    hb = m.prepare_folds(part)
    db = m.prepare_folds_from_labels(labels)
    if kind == "float_nan":
        assert len(db.labels) == len(part.folds_dict)
        assert sum(1 for v in db.labels if v != v) == 3            # three NaN rows, three folds of one row
        assert all(a == b or (a != a and b != b) for a, b in zip(db.labels, part.folds_dict))
    else:
        assert db.labels == list(part.folds_dict)
    assert np.array_equal(db.host_offsets, hb.host_offsets)
    assert bool((db.idx == hb.idx).all()) and np.array_equal(db.nz_val, hb.nz_val)
    a, _ = m.training_XTX_batched(hb)
    b, _ = m.training_XTX_batched(db)
    assert bool((a == b).all())


@pytest.mark.parametrize("N,L,bad", [(6000, 5000, -5), (6000, 5000, -(2 ** 62)), (3000, 40, -1), (6000, 5000, 5000)])
def test_device_partitioner_refuses_out_of_range_labels(amd, N, L, bad):
    """A label outside [0, n_labels) -- negative ones included, on the many-label radix route too --
    raises the ValueError, through the class (checked on the host before any kernel runs) and
    through the C ABI alone (the error flag is set, nothing is written out of bounds, the call
    returns)."""
    import torch

    from cvmatrix_amd import _lib

    rng = np.random.default_rng(N + L)
    labels = rng.integers(0, L, size=N)
    labels[N // 2] = bad                      # (directly in front of / behind valid rows in the sorted order)
    m = amd.CVMatrix()
    m.fit(rng.random((N, 8)))
    with pytest.raises(ValueError, match="fold labels"):
        m.prepare_folds_from_labels(labels, n_labels=L)
    lib = _lib.load()
    dev = m.device
    lab = torch.from_numpy(labels).to(dev)
    guard = 4096                              # canaries around the outputs: nothing outside them is touched
    idx = torch.full((N + 2 * guard,), -7, dtype=torch.int64, device=dev)
    offs = torch.full((L + 1 + 2 * guard,), -7, dtype=torch.int64, device=dev)
    first = torch.full((L + 2 * guard,), -7, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.cvm_partition_workspace_bytes(N, L)), dtype=torch.uint8, device=dev)
    rc = lib.cvm_partition_labels(lab.data_ptr(), N, L, idx[guard:].data_ptr(), offs[guard:].data_ptr(),
                                  first[guard:].data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel(), 0)
    torch.cuda.synchronize()
    assert rc == 0 and int(err.item()) != 0
    for t, n in ((idx, N), (offs, L + 1), (first, L)):
        assert bool((t[:guard] == -7).all()) and bool((t[guard + n:] == -7).all())


def _empty_rank_worker(rank, world, port, tmp):
    import os
    import sys

    import torch
    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cvmatrix_amd import CVMatrix
        from cvmatrix_amd.distributed import ShardedCVMatrix

        torch.cuda.set_device(0)
        rng = np.random.default_rng(19)
        N, K, M = 3000, 66, 2
        X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N) + 0.01
        full = CVMatrix(lazy_fit=False)
        full.fit(X, Y, w)
        rows = np.arange(N) if rank == 0 else np.zeros(0, dtype=np.int64)     # rank 1 owns nothing
        for lazy in (False, True):
            sh = ShardedCVMatrix(mode="row_sharded", lazy_fit=lazy)
            sh.fit(X[rows], Y[rows], w[rows])
            # every rank asks for the matrices (the lazy exchange is collective); rank 1 has no fold
            assert torch.allclose(sh.XTX, full.XTX, rtol=1e-12, atol=1e-12)
            assert torch.allclose(sh.XTY, full.XTY, rtol=1e-12, atol=1e-12)
            if rank == 0:
                folds = [np.arange(i, N, 3) for i in range(3)]
                (a, b), sa = sh.training_XTX_XTY_batched(folds)
                (c, d), sc = full.training_XTX_XTY_batched(folds)
                assert torch.allclose(a, c, rtol=1e-10, atol=1e-10) and torch.allclose(b, d, rtol=1e-10, atol=1e-10)
        open(os.path.join(tmp, f"ok_empty_{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_a_rank_without_rows_takes_part_in_the_exchange(amd, tmp_path):
    """More ranks than folds (strong scaling of 10 folds on 16 GPUs, or any rank whose shard is empty):
    such a rank fits zero rows -- zeros, no kernel -- and still issues the one collective, so the
    other ranks neither hang nor get a wrong sum."""
    import os

    import torch.multiprocessing as mp

    port = 29300 + (os.getpid() % 1500)
    mp.spawn(_empty_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok_empty_0").exists() and (tmp_path / "ok_empty_1").exists()


def _sharded_worker(rank, world, port, tmp, mode):
    import os
    import sys

    import torch
    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cvmatrix_amd import CVMatrix
        from cvmatrix_amd.distributed import ShardedCVMatrix

        torch.cuda.set_device(0)
        rng = np.random.default_rng(9)
        N, K, M, P = 8000, 130, 4, 8
        X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
        w[::13] = 0.0
        full = CVMatrix()
        full.fit(X, Y, w)
        if mode == "row_sharded":
            rows = np.arange(N).reshape(world, N // world)[rank]
            sh = ShardedCVMatrix(mode="row_sharded")
            sh.fit(X[rows], Y[rows], w[rows])
            local = [np.arange(i, rows.size, P // world) for i in range(P // world)]
            glob = [rows[v] for v in local]
        else:
            sh = ShardedCVMatrix(mode="replicated")
            sh.fit(X, Y, w)
            all_folds = [np.arange(i, N, P) for i in range(P)]
            mine = sh.my_folds([len(v) for v in all_folds])
            local = glob = [all_folds[f] for f in mine]
        assert torch.allclose(sh.XTX, full.XTX, rtol=1e-12, atol=1e-12)
        assert torch.allclose(sh.XTY, full.XTY, rtol=1e-12, atol=1e-12)
        if mode == "row_sharded":
            # one-sweep variant on every rank's own rows (what bench.py times next to the headline):
            # local validation Grams, all-reduced full-data matrices
            sw = ShardedCVMatrix(mode="row_sharded")
            sw.fit(X[rows], Y[rows], w[rows], folds=local)
            assert torch.allclose(sw.XTX, full.XTX, rtol=1e-12, atol=1e-12)
            (e, f_), se = sw.training_XTX_XTY_batched(sw.sweep_folds)
            (c0, d0), sc0 = full.training_XTX_XTY_batched(glob)
            assert torch.allclose(e, c0, rtol=1e-10, atol=1e-10) and torch.allclose(f_, d0, rtol=1e-10, atol=1e-10)
            for s, t_ in zip(se, sc0):
                assert torch.allclose(s, t_, rtol=1e-10, atol=1e-12)
        (a, b), sa = sh.training_XTX_XTY_batched(local)
        (c, d), sc = full.training_XTX_XTY_batched(glob)
        assert torch.allclose(a, c, rtol=1e-10, atol=1e-10) and torch.allclose(b, d, rtol=1e-10, atol=1e-10)
        for s, t in zip(sa, sc):
            assert torch.allclose(s, t, rtol=1e-10, atol=1e-12)
        # lazy fit (what bench.py times): the exchange moves to the first batched call, which every
        # rank makes; row-sharded: the rank's folds partition its rows -> one sweep + all-reduce
        lz = ShardedCVMatrix(mode=mode, lazy_fit=True)
        lz.fit(X[rows], Y[rows], w[rows]) if mode == "row_sharded" else lz.fit(X, Y, w)
        assert lz._pending
        (a2, b2), sa2 = lz.training_XTX_XTY_batched(local)
        assert not lz._pending and (lz._sweep is not None) == (mode == "row_sharded")
        assert torch.allclose(a2, c, rtol=1e-10, atol=1e-10) and torch.allclose(b2, d, rtol=1e-10, atol=1e-10)
        for s, t in zip(sa2, sc):
            assert torch.allclose(s, t, rtol=1e-10, atol=1e-12)
        assert torch.allclose(lz.XTX, full.XTX, rtol=1e-12, atol=1e-12)
        open(os.path.join(tmp, f"ok_{mode}_{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["row_sharded", "replicated"])
def test_two_ranks_share_one_gpu(amd, tmp_path, mode):
    """ShardedCVMatrix with two processes (gloo rendezvous, both on cuda:0): row-sharded fit +
    one all-reduce of the contiguous [G | H | gstats] buffer, or replicated fit + one broadcast;
    every rank's folds equal the single-process result.  (On the 8-GPU node the same code runs
    with backend "nccl" = RCCL, one rank per GPU.)"""
    import os

    import torch.multiprocessing as mp

    port = 29600 + (os.getpid() % 1500) + (7 if mode == "replicated" else 0)
    mp.spawn(_sharded_worker, args=(2, port, str(tmp_path), mode), nprocs=2, join=True)
    assert (tmp_path / f"ok_{mode}_0").exists() and (tmp_path / f"ok_{mode}_1").exists()


@pytest.mark.parametrize("mode,path", [("row_sharded", "sweep"), ("replicated", "sweep"),
                                       ("row_sharded", "two_stage")])
def test_bench_command_two_ranks_strong_scaling(amd, mode, path):
    """The driver's multi-GPU command line, end to end: `python -m torch.distributed.run
    --nproc-per-node 2 bench.py --gpus 2 ...` (gloo rendezvous, both ranks on cuda:0 -- a
    1-GPU box; the 8-GPU node runs the same command over RCCL).  Strong scaling: the folds
    of ONE problem dealt over the ranks; the JSON line names the same global workload as the
    single-process run and carries the in-run parity gate (a fold recomputed from scratch)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    port = 29900 + (os.getpid() % 1000) + {"row_sharded": 0, "replicated": 3}[mode] + (5 if path != "sweep" else 0)
    common = ["--rows", "4000", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--mode", mode,
              "--path", path]
    two = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
         "--gpus", "2", *common], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-2000:]
    line2 = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", *common], env=env,
                         cwd=root, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    line1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    for line, n in ((line1, 1), (line2, 2)):
        assert line["n_gpus"] == n and line["scaling"] == "strong" and line["unit"] == "folds/s"
        assert line["parity"].startswith("ok"), line["parity"]
        assert line["roofline"]["bound"] == "mfma" and line["value"] > 0
    # the same global problem on both lines
    assert line1["metric"] == line2["metric"]
    assert line1["config"]["workload"] == line2["config"]["workload"]
    assert line2["scaling_ceiling_vs_1gpu"] == 2.0 and line1["scaling_ceiling_vs_1gpu"] == 1.0


def test_bench_plain_run_dumps_the_timed_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run (no --full) times exactly --steps steps, prints the headline line without
    running the parity gate, and --dump-outputs writes what the timed path returned in its last step: every fold's
    XTX, XTY and statistics, here checked against the oracle on the same seeded inputs."""
    import json
    import os
    import subprocess
    import sys

    import bench

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--rows", "4000", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(d)], cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "folds/s" and line["dtype"] == "f64" and line["parity"] == "not checked"
    assert line["two_stage_ms_per_step"] is None and line["cpu_baseline"] is None and line["other_workloads"] is None
    N, K, M, P = 4000, 512, 16, 10
    X, Y, w = bench.synth(N, K, M, np.float64, 42)
    o = OracleCVMatrix(True, True, True, True, ddof=1)
    o.fit(X, Y, w)
    op = OraclePartitioner(np.arange(N) % P)
    got = {n: np.load(d / f"{n}.npy") for n in ("XTX", "XTY", "mean_X", "std_X", "mean_Y", "std_Y")}
    assert all(a.dtype == np.float64 for a in got.values())
    for i, f in enumerate(op.folds_dict):
        (rx, ry), rst = o.training_XTX_XTY(op.get_validation_indices(f))
        assert_normwise(got["XTX"][i], rx, TOL, f"fold {f} XTX")
        assert_normwise(got["XTY"][i], ry, TOL, f"fold {f} XTY")
        assert_stats(tuple(got[n][i] for n in ("mean_X", "std_X", "mean_Y", "std_Y")), rst, 1e-10, f"fold {f}")


def test_bench_plain_command_starts_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` with NO launcher in front -- the form the driver uses for `--gpus 1` -- starts
    `torch.distributed.run` itself as a child process (the parent never touches the GPU), relays rank 0's one JSON
    line and leaves with the child's exit code (the reference's harness is one command too,
    benchmarks/benchmark.py:293-308).  Two ranks on cuda:0 over gloo here; RCCL on a multi-GPU node."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(CVM_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--rows", "4000", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline"], env=env, cwd=root, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["parity"].startswith("ok"), line
    # a launcher whose rank count disagrees with --gpus is refused, not silently run
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--rows", "4000", "--steps", "1",
                          "--warmup", "0", "--no-cpu-baseline"], env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "must agree" in bad.stderr


def test_multi_gpu_smoke_two_ranks_on_one_gpu():
    """``__graft_entry__.rccl_smoke`` -- what ``smoke()`` starts on a box with two GPUs, over RCCL -- run here by
    two ranks that share cuda:0 over gloo: every fold of every rank against the oracle, row-sharded (one
    all-reduce) and replicated (one broadcast)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(29700 + os.getpid() % 200),
                        os.path.join(root, "__graft_entry__.py"), "rccl_smoke"], env=env, cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rccl smoke ok (gloo, 2 ranks)" in r.stdout


@pytest.mark.parametrize("K,M,route", [(4, 1, "units"), (64, 3, "units"), (132, 1, "units"), (260, 34, "units"),
                                       (516, 16, "units"), (128, 5, "many"), (388, 0, "many"), (130, 2, "units")])
def test_float32_shape_sweep(amd, K, M, route):
    """float32: K a multiple of 4 takes the LDS-DMA kernel (any M: the Y tile rows go by
    dwords), other K the general kernel (the last case); a few large folds and many mid-size
    folds; against the float64 oracle on the float32-rounded inputs, error bounded by a small
    multiple of float32 rounding of the sums involved: at most twice the error of the reference's
    algorithm in NumPy float32 on the same inputs plus FP32_FLOOR."""
    rng = np.random.default_rng(500 + K + M)
    N = 9000
    X = (rng.random((N, K)) + 0.1).astype(np.float32)
    Y = rng.random((N, M)).astype(np.float32) if M else None
    w = rng.random(N).astype(np.float32)
    w[rng.choice(N, 300, replace=False)] = 0
    perm = rng.permutation(N)
    if route == "units":
        folds = [perm[:2500], perm[2500:4000], perm[4000:]]
    else:
        folds = [perm[i:i + 75] for i in range(0, N, 75)]
    for flags in [(True,) * 4, (False,) * 4]:
        m = amd.CVMatrix(*flags, dtype=np.float32)
        o = OracleCVMatrix(*flags, dtype=np.float64)
        o32 = OracleCVMatrix(*flags, dtype=np.float32)      # the reference's own float32 arithmetic
        m.fit(X, Y, w)
        o.fit(X.astype(np.float64), None if Y is None else Y.astype(np.float64), w.astype(np.float64))
        o32.fit(X, Y, w)
        assert_fp32_like_reference(m.XTX, o.XTX, o32.XTX, "fit XTX", floor=FP32_FLOOR)
        if M:
            (bx, by), bst = m.training_XTX_XTY_batched(folds)
        else:
            bx, bst = m.training_XTX_batched(folds)
        for f in (0, len(folds) - 1):
            if M:
                (rx, ry), rst = o.training_XTX_XTY(folds[f])
                (sx, sy), _ = o32.training_XTX_XTY(folds[f])
                assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY", floor=FP32_FLOOR)
            else:
                rx, rst = o.training_XTX(folds[f])
                sx, _ = o32.training_XTX(folds[f])
            assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX", floor=FP32_FLOOR)
            for a_, b_ in zip(bst, rst):
                assert (a_ is None) == (b_ is None)
                if b_ is not None:
                    np.testing.assert_allclose(to_np(a_[f]).astype(np.float64), b_, rtol=F32_STAT_RTOL)
            t = bx[f]
            assert bool((t == t.T).all())


# ---------------------------------------------------------------- lazy fit (the default)
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("flags", [(True,) * 4, (False,) * 4, (True, False, False, True)])
def test_lazy_fit_one_sweep_equals_eager_and_oracle(amd, weighted, flags):
    """fit() leaves the full-data matrices pending; a batched call whose folds partition the rows
    forms them as the sum of the folds' validation matrices (one sweep).  Same results as the
    eager two-stage path (to rounding) and as the oracle (1e-10)."""
    rng = np.random.default_rng(77)
    N, K, M, P = 6000, 136, 6, 5
    X, Y = rng.random((N, K)), rng.random((N, M))
    w = rng.random(N) if weighted else None
    if weighted:
        w[::17] = 0.0
    folds = [np.arange(N)[np.arange(N) % P == f] for f in range(P)]
    lz = amd.CVMatrix(*flags, lazy_fit=True)
    eg = amd.CVMatrix(*flags, lazy_fit=False)
    lz.fit(X, Y, w)
    eg.fit(X, Y, w)
    assert lz._pending and not eg._pending
    (a, b), sa = lz.training_XTX_XTY_batched(folds)
    assert not lz._pending and lz._sweep is not None
    (c, d), sc = eg.training_XTX_XTY_batched(folds)
    assert_normwise(a, to_np(c), 1e-11, "lazy vs eager XTX")
    assert_normwise(b, to_np(d), 1e-11, "lazy vs eager XTY")
    assert_normwise(lz.XTX, to_np(eg.XTX), 1e-12, "full-data XTX")
    assert_normwise(lz.XTY, to_np(eg.XTY), 1e-12, "full-data XTY")
    o = OracleCVMatrix(*flags)
    o.fit(X, Y, w)
    for f in (0, P - 1):
        (rx, ry), rst = o.training_XTX_XTY(folds[f])
        assert_normwise(a[f], rx, TOL, "XTX")
        assert_normwise(b[f], ry, TOL, "XTY")
        assert_stats(tuple(None if s is None else s[f] for s in sa), rst, TOL)
    # the same batch again (no refit): the partials are reused; a refit makes it pending again
    batch = lz.prepare_folds(folds)
    lz.fit(X, Y, w)
    (a3, b3), _ = lz.training_XTX_XTY_batched(batch)
    (a4, b4), _ = lz.training_XTX_XTY_batched(batch)
    assert torch_equal(a3, a4) and torch_equal(b3, b4) and torch_equal(a3, a)


@pytest.mark.parametrize("dtype,N,K,M,P,weighted", [
    (np.float64, 9000, 136, 6, 5, True), (np.float64, 9000, 260, 0, 3, False), (np.float64, 12000, 512, 16, 10, True),
    (np.float64, 20000, 132, 40, 16, True), (np.float64, 20000, 132, 2, 17, True), (np.float64, 9000, 135, 3, 4, True),
    (np.float32, 9000, 136, 5, 6, True), (np.float32, 9000, 516, 1, 4, False), (np.float32, 9000, 130, 3, 4, True)])
def test_sweep_all_one_call_equals_the_two_calls(amd, dtype, N, K, M, P, weighted):
    """cvm_sweep_all (a lazy fit followed by a batched call over a partition: the folds' updates
    stay in registers while G is formed, two finalize launches) against cvm_sweep_fit +
    cvm_sweep_folds (fit(folds=...), then the batched call): the same bits in the full-data
    matrices, the column sums, every fold's matrices and statistics -- for aligned rows with up to
    16 folds (the merged kernels) and beyond (17 folds, K * itemsize not a multiple of 16: the
    separate kernels behind the same entry point); and against the oracle."""
    rng = np.random.default_rng(N + K + P)
    X = rng.random((N, K)).astype(dtype)
    Y = rng.random((N, M)).astype(dtype) if M else None
    w = rng.random(N).astype(dtype) if weighted else None
    if weighted:
        w[::13] = 0
    part = amd.Partitioner(rng.integers(0, P, N))
    for flags in ((True,) * 4, (False,) * 4, (True, False, False, True)):
        one = amd.CVMatrix(*flags, dtype=dtype, lazy_fit=True)
        two = amd.CVMatrix(*flags, dtype=dtype, lazy_fit=False)
        one.fit(X, Y, w)
        two.fit(X, Y, w, folds=part)
        assert one._pending
        if M:
            (ax, ay), ast = one.training_XTX_XTY_batched(part)
            (bx, by), bst = two.training_XTX_XTY_batched(two.sweep_folds)
            assert torch_equal(ay, by)
        else:
            ax, ast = one.training_XTX_batched(part)
            bx, bst = two.training_XTX_batched(two.sweep_folds)
        assert not one._pending and one._sweep is not None
        assert torch_equal(ax, bx)
        assert torch_equal(one.XTX, two.XTX) and torch_equal(one._gstats, two._gstats)
        if M:
            assert torch_equal(one.XTY, two.XTY)
        for s_, t_ in zip(ast, bst):
            assert (s_ is None) == (t_ is None)
            if s_ is not None:
                assert torch_equal(s_, t_)
        assert bool((ax[0] == ax[0].transpose(0, 1)).all())
        # matrices of one kind only, from a fresh pending fit
        one.fit(X, Y, w)
        cx, _ = one.training_XTX_batched(part)
        assert torch_equal(cx, ax)
        if M:
            one.fit(X, Y, w)
            cy, _ = one.training_XTY_batched(part)
            two.fit(X, Y, w, folds=part)
            dy, _ = two.training_XTY_batched(two.sweep_folds)
            assert torch_equal(cy, dy)
        # single folds afterwards are served from the same partials
        keys = list(part.folds_dict)
        o = OracleCVMatrix(*flags, dtype=np.float64)
        o.fit(X.astype(np.float64), None if Y is None else Y.astype(np.float64), None if w is None else w.astype(np.float64))
        tol = TOL if dtype is np.float64 else 3e-4
        for f in (0, P - 1):
            v = part.get_validation_indices(keys[f])
            if M:
                (rx, ry), rst = o.training_XTX_XTY(v)
                assert_normwise(ay[f].double(), ry, tol, "XTY")
            else:
                rx, rst = o.training_XTX(v)
            assert_normwise(ax[f].double(), rx, tol, "XTX")
        assert_normwise(one.XTX.double(), o.XTX, 1e-12 if dtype is np.float64 else 2e-5, "full-data XTX")


@pytest.mark.parametrize("plan", ["7,2", "3,5", "1,4", "2,1"])
def test_forced_split_plans(plan):
    """The two classes of work items (off-diagonal / diagonal tiles) under row-split plans the
    planner would not pick for these shapes, both orders of s_off and s_diag: two-stage path, sweep
    and one-fold calls against the oracle at 1e-10 (tests/forced_plan_check.py in a subprocess --
    the library reads CVM_FORCE_SPLITS once)."""
    import subprocess

    env = dict(os.environ, CVM_FORCE_SPLITS=plan)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "forced_plan_check.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "worst norm-wise error" in r.stdout


@pytest.mark.parametrize("switch", ["CVM_NO_FUSED=1", "CVM_FORCE_FALLBACK=1", "CVM_NO_SWEEP_MERGE=1", "CVM_NO_DIRECT=1",
                                    "CVM_NO_COMPACT=1", "CVM_NO_INLINE_STATS=1", "CVM_SERVE_LOOPS=0", "CVM_PAD=0",
                                    "CVM_SMALL_MAXN=128", "CVM_MID_TILE=0", "CVM_MID_MINN=1", "CVM_MID_MAXN=1000",
                                    "CVM_FUSED_PREPASS=1", "CVM_FUSED_ORDER=1"])
def test_route_forcing_switches(switch):
    """One pass of tools/route_matrix.sh inside the suite: every route-forcing switch of the library
    (read once per process, hence a subprocess each) over tests/forced_plan_check.py -- two-stage
    path, sweep, per-fold calls, mid-size folds (tile kernel / fused epilogue / two-stage), folds of a few rows
    (tile kernel / whole-rows kernel) -- against the oracle at 1e-10."""
    import subprocess

    k, v = switch.split("=")
    env = dict(os.environ, **{k: v})
    env.pop("CVM_FORCE_SPLITS", None)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "forced_plan_check.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


_FUSED_TIMEOUT_CODE = """
import numpy as np, torch, sys
sys.path.insert(0, %(root)r)
from cvmatrix_amd import CVMatrix
from oracle.cvmatrix_oracle import OracleCVMatrix
mode = %(mode)d
worst = 0.0
# (a hundred folds each: with few work items the planner cuts the folds' rows into splits and the call takes the
#  route with partials, which waits for nothing)
# (folds of 300 rows and more: the fused Gram route, which forms its statistics in the launch)
for dtype, N, K, M, nv, seed in ((np.float64, 30000, 516, 16, 300, 1),
                                 (np.float64, 40000, 260, 2, 400, 2), (np.float32, 33000, 260, 4, 330, 3)):
    rng = np.random.default_rng(seed)
    X, Y, w = rng.random((N, K)) + 0.1, rng.random((N, M)), rng.random(N) + 0.01
    perm = rng.permutation(N)
    folds = [np.sort(perm[i:i + nv]) for i in range(0, N, nv)]
    o = OracleCVMatrix(); o.fit(X, Y, w)
    m = CVMatrix(dtype=dtype, lazy_fit=False); m.fit(X, Y, w)
    (bx, by), st = m.training_XTX_XTY_batched(folds)
    status = m.fold_status()
    # (the route that waits is taken when the planner gives every fold one unit; the first problem is sized so
    #  that it does, the others may or may not -- status 0 then, and every fold must be right)
    tol = 1e-10 if dtype is np.float64 else 2e-4
    for f in list(range(0, 12)) + list(range(12, len(folds), 7)):
        (rx, ry), rst = o.training_XTX_XTY(folds[f])
        gx, gy = bx[f].double().cpu().numpy(), by[f].double().cpu().numpy()
        if mode == 3 and status == 1 and f %% 3 == 0:
            # the retry launch was made to give up too: every off-diagonal tile of these folds is poisoned,
            # nothing of them passes for a number
            assert np.isnan(gx).any(), f
            continue
        assert np.isfinite(gx).all() and np.isfinite(gy).all(), f
        worst = max(worst, np.abs(gx - rx).max() / np.abs(rx).max(), np.abs(gy - ry).max() / np.abs(ry).max())
        assert (gx == gx.T).all()
        for g_, r_ in zip(st, rst):
            worst = max(worst, np.abs(g_[f].double().cpu().numpy() - r_).max() / np.abs(r_).max())
    assert worst <= tol, (dtype, worst)
    print("status", status)
    first = seed == 1
    if mode == 1: assert status == 2 if first else status in (0, 2), status
    if mode == 2: assert status in (0, 2), status
    if mode == 3: assert status == 1 if first else status in (0, 1), status
print("timeouts handled ok")
"""


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_a_flag_wait_that_gives_up_is_recomputed_and_reported(mode):
    """Mid-size folds form their statistics inside the Gram launch: off-diagonal work items wait for flags that
    diagonal items of the same launch raise (wgram4.hpp).  The wait is bounded, and what happens when it gives
    up is tested here by making it give up (``CVM_FUSED_TEST_TIMEOUT``): 1 = the off-diagonal items of every
    third fold give up at once, 2 = a spin limit of four polls (they give up whenever a flag is not up yet),
    3 = like 1 and the retry launch is made to give up as well.  Modes 1 and 2: every result is the oracle's
    (the items were recomputed by the second launch of the same call), ``fold_status()`` says 2 where items
    were recomputed.  Mode 3: status 1 and NaN in the affected folds -- never a finite wrong number.  The
    reference's contract: cvmatrix.py:754-896 raises or returns correct numbers."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _FUSED_TIMEOUT_CODE % {"root": root, "mode": mode}
    env = dict(os.environ, CVM_FUSED_TEST_TIMEOUT=str(mode))
    # (the test is about the route that waits: a switch of tools/route_matrix.sh that takes the call elsewhere is lifted)
    for k in ("CVM_FORCE_SPLITS", "CVM_NO_FUSED", "CVM_FORCE_FALLBACK", "CVM_FUSED_PREPASS", "CVM_MID_TILE",
              "CVM_MID_MINN", "CVM_MID_MAXN"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    assert "timeouts handled ok" in r.stdout


def test_fused_route_next_to_a_kernel_that_holds_the_compute_units(amd):
    """The same route while another stream keeps the compute units busy (a chain of large matrix products):
    workgroups of the Gram launch then start late and out of step, which is when an inter-workgroup wait shows
    what it is made of.  Results must be bit for bit those of the quiet device, and the status word must not
    report poisoned outputs."""
    import torch

    rng = np.random.default_rng(11)
    N, K, M, nv = 30000, 516, 16, 300
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N) + 0.01
    folds = [np.arange(f, N, N // nv)[:nv] for f in range(N // nv)]
    m = amd.CVMatrix(lazy_fit=False)
    m.fit(X, Y, w)
    b = m.prepare_folds(folds)
    (qx, qy), _ = m.training_XTX_XTY_batched(b)
    qx, qy = qx.clone(), qy.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    A = torch.rand((6144, 6144), device="cuda", dtype=torch.float32)
    for rep in range(3):
        with torch.cuda.stream(side):
            C_ = A
            for _ in range(12):
                C_ = (C_ @ A) * 1e-4
        (bx, by), _ = m.training_XTX_XTY_batched(b)
        torch.cuda.synchronize()
        assert torch.equal(bx, qx) and torch.equal(by, qy), rep
    assert m.fold_status() in (0, 2)


def test_wide_matrices_k8192_k16384():
    """K = 8192 and 16384 (G of 0.27 / 1 GB in float32, 2 GB in float64), few folds, and an odd
    K = 8191 with 40 folds: the fold stage against a from-scratch float64 computation of the centred /
    scaled training-set matrices on the device (tools/big_k_check.py; float64 1e-10, float32 1e-3)."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "big_k_check.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("XTX err") == 4, r.stdout


@pytest.mark.parametrize("dtype,K,M,nv", [(np.float64, 4096, 2, 100), (np.float64, 1024, 4, 44), (np.float32, 1024, 3, 60),
                                          (np.float32, 512, 1, 45)])
def test_direct_route_beyond_one_chunk_by_the_default_table(amd, dtype, K, M, nv):
    """Folds of 33 ... 128 rows where the library's own table (small_route_limit, host.hpp) sends
    them to the direct kernels in several 32-row chunks -- float64 K >= 4096 up to 128 rows,
    768 <= K < 4096 up to 48; float32 up to 64 / 48 -- against the oracle, ragged folds, weights
    with zeros."""
    rng = np.random.default_rng(K + nv)
    P = 5
    N = P * nv + 40
    X = rng.random((N, K)).astype(dtype)
    Y = rng.random((N, M)).astype(dtype)
    w = rng.random(N).astype(dtype)
    w[rng.choice(N, N // 10, replace=False)] = 0
    perm = rng.permutation(N)
    sizes = [nv, nv - 7, nv, 33, nv - 1]
    folds, o = [], 0
    for n in sizes:
        folds.append(np.sort(perm[o:o + n])); o += n
    flags = (True, True, True, True)
    if dtype is np.float64:
        m, _ = _compare_with_oracle(amd, X, Y, w, folds, flags)
        (bx, _), _ = m.training_XTX_XTY_batched(folds)
    else:
        m = amd.CVMatrix(*flags, dtype=np.float32)
        m.fit(X, Y, w)
        o = OracleCVMatrix(*flags)
        o.fit(X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64))
        o32 = OracleCVMatrix(*flags, dtype=np.float32)
        o32.fit(X, Y, w)
        (bx, by), _ = m.training_XTX_XTY_batched(folds)
        for f, v in enumerate(folds):
            (rx, ry), _ = o.training_XTX_XTY(v)
            (sx, sy), _ = o32.training_XTX_XTY(v)
            assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX")
            assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY")
    for f in range(P):
        assert bool((bx[f] == bx[f].T).all())


@pytest.mark.parametrize("dtype,K,M,sizes", [
    (np.float64, 512, 16, (100, 8, 9, 255, 256, 17)),      # the bench's mid-size shape; the route's edges at K = 512
    (np.float64, 66, 2, (40, 12, 64, 65)),                 # one tile column past the first panel
    (np.float64, 130, 40, (33, 48, 100, 16)),              # M > 16: XTY-only items; K just past two panels
    (np.float64, 1030, 4, (16, 60, 200, 31)),              # K = 1024 + one piece: 17 panels, from 16 rows
    (np.float64, 2048, 2, (16, 120)),                      # the widest shape of the route
    (np.float64, 384, 0, (90, 10, 130)),                   # no Y
    (np.float32, 512, 16, (100, 8, 320, 47)),
    (np.float32, 260, 20, (64, 9, 150)),
    (np.float32, 1024, 4, (8, 100, 319)),
])
def test_mid_tile_route_shapes(amd, dtype, K, M, sizes):
    """Batches of folds of 8 / 16 to a few hundred rows take mid_tile_kernel (host.hpp: mid_default_minn /
    _maxn): every flag set that changes its finish, weights with zeros and none, ragged folds incl. the
    sizes at the route's limits and partial last k-steps, against the oracle (float32: the oracle's own
    float32 run as the yardstick); exact symmetry of every XTX."""
    rng = np.random.default_rng(K * 7 + M)
    N = sum(sizes) + 57
    X = (rng.standard_normal((N, K)) + 0.25).astype(dtype)
    Y = rng.random((N, M)).astype(dtype) if M else None
    w = rng.random(N).astype(dtype)
    w[rng.choice(N, N // 12, replace=False)] = 0
    perm = rng.permutation(N)
    folds, o_ = [], 0
    for n in sizes:
        folds.append(np.sort(perm[o_:o_ + n])); o_ += n
    for flags, wt in (((True,) * 4, w), ((False,) * 4, w), ((True, False, False, True), None), ((False, True, True, False), w)):
        if dtype is np.float64:
            m, _ = _compare_with_oracle(amd, X, Y, wt, folds, flags)
            bx = (m.training_XTX_XTY_batched(folds)[0][0] if M else m.training_XTX_batched(folds)[0])
        else:
            m = amd.CVMatrix(*flags, dtype=np.float32)
            m.fit(X, Y, wt)
            o = OracleCVMatrix(*flags)
            o.fit(X.astype(np.float64), None if Y is None else Y.astype(np.float64), None if wt is None else wt.astype(np.float64))
            o32 = OracleCVMatrix(*flags, dtype=np.float32)
            o32.fit(X, Y, wt)
            (bx, by), _ = m.training_XTX_XTY_batched(folds)
            for f, v in enumerate(folds):
                (rx, ry), _ = o.training_XTX_XTY(v)
                (sx, sy), _ = o32.training_XTX_XTY(v)
                assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX")
                assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY")
        for f in range(len(folds)):
            assert bool((bx[f] == bx[f].T).all())


@pytest.mark.parametrize("K,M,sizes,reps", [
    (1024, 3, (16, 1, 0, 7, 16, 2, 9), 1),          # 32 blocks x up to 16 workgroup sets; ragged folds incl. an empty one
    (1024, 0, (5,) * 70, 1),                         # more folds than workgroup sets: several folds per workgroup; no Y
    (2048, 2, (16, 3, 12, 16, 8, 1, 16, 4, 11), 1),  # 128 blocks, two workgroup sets
    (4096, 1, (16, 15, 2, 9), 2),                    # every block of the chip's 512; the diagonal tile in every wave position
    (1024, 20, (16, 4, 9, 16, 1), 1),                # M > 16: XTY by the tile kernel's panels behind the resident XTX
    (1024, 2, (32, 17, 1, 25, 0, 32, 20, 9), 1),     # folds of 17 to 32 rows: operand blocks of 36 rows, one tile per step
    (2048, 1, (31, 32, 18, 32), 2),
])
def test_resident_route_float32(amd, K, M, sizes, reps):
    """float32 XTX of batches of folds of at most 32 rows, K a multiple of 1024: res8_apply_kernel (resident.hpp) -- G in
    the register files of the whole chip, every tile computed directly from wave-private LDS-DMA operands behind counted
    waits.  Every flag set that changes the operand block, weights with zeros and none, ragged folds, against the float64
    oracle with the oracle's own float32 run as the yardstick; exact symmetry; bit-identical repetitions (a misplaced
    wait would show as rare wrong tiles)."""
    import torch
    from cvmatrix_amd import _lib

    lib = _lib.load()
    assert lib.cvm_debug_resident(1) == 0        # wherever the shape allows (the default rule: K >= 4096, >= 32 folds per batch)
    try:
        _resident_case(amd, K, M, sizes, reps, torch)
    finally:
        lib.cvm_debug_resident(2)


def _resident_case(amd, K, M, sizes, reps, torch):
    rng = np.random.default_rng(K + M)
    N = sum(sizes) + 40
    X = (rng.standard_normal((N, K)) * 0.5 + 0.25).astype(np.float32)
    Y = rng.random((N, M)).astype(np.float32) if M else None
    w = rng.random(N).astype(np.float32)
    w[rng.choice(N, N // 10, replace=False)] = 0
    perm = rng.permutation(N)
    folds, o_ = [], 0
    for n in sizes:
        folds.append(np.sort(perm[o_:o_ + n])); o_ += n
    check = range(len(folds)) if len(folds) <= 9 else (0, 1, 17, 33, len(folds) - 1)
    cases = (((True,) * 4, w), ((False,) * 4, w), ((True, False, False, True), None), ((False, True, True, False), w))
    for flags, wt in (cases if K < 4096 else cases[:1]):
        m = amd.CVMatrix(*flags, dtype=np.float32)
        m.fit(X, Y, wt)
        o = OracleCVMatrix(*flags)
        o.fit(X.astype(np.float64), None if Y is None else Y.astype(np.float64), None if wt is None else wt.astype(np.float64))
        o32 = OracleCVMatrix(*flags, dtype=np.float32)
        o32.fit(X, Y, wt)
        bx = m.training_XTX_XTY_batched(folds)[0][0] if M else m.training_XTX_batched(folds)[0]
        by = m.training_XTX_XTY_batched(folds)[0][1] if M else None
        for f in check:
            rx = o.training_XTX(folds[f])[0]
            sx = o32.training_XTX(folds[f])[0]
            assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX")
            if M:
                ry = o.training_XTX_XTY(folds[f])[0][1]
                sy = o32.training_XTX_XTY(folds[f])[0][1]
                assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY")
        for f in range(len(folds)):
            assert bool((bx[f] == bx[f].T).all()), f
        for _ in range(reps):
            bx2 = m.training_XTX_XTY_batched(folds)[0][0] if M else m.training_XTX_batched(folds)[0]
            assert torch.equal(bx, bx2)


def test_resident_route_is_the_default_for_wide_float32_batches(amd):
    """The library's own rule (cvm_debug_resident mode 2): float32, K = 4096, 40 folds of at most 16 rows -> res8_apply_kernel
    (BASELINE's C5-hbm shape).  The default call must be bit-identical to the forced route (same kernel), within the float32 gate
    of the oracle, exactly symmetric, and agree with the tile kernel (mode 0) to float32 rounding."""
    import torch
    from cvmatrix_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(4096)
    K, M, P = 4096, 1, 40
    sizes = rng.integers(1, 17, P)
    N = int(sizes.sum()) + 30
    X = (rng.standard_normal((N, K)) * 0.5 + 0.25).astype(np.float32)
    Y = rng.random((N, M)).astype(np.float32)
    w = rng.random(N).astype(np.float32)
    perm = rng.permutation(N)
    folds, o_ = [], 0
    for n in sizes:
        folds.append(np.sort(perm[o_:o_ + int(n)])); o_ += int(n)
    m = amd.CVMatrix(dtype=np.float32)
    m.fit(X, Y, w)
    (bx, by), _ = m.training_XTX_XTY_batched(folds)                      # the default rule
    try:
        assert lib.cvm_debug_resident(1) == 0
        (fx, fy), _ = m.training_XTX_XTY_batched(folds)
        assert lib.cvm_debug_resident(0) == 0
        (tx, ty), _ = m.training_XTX_XTY_batched(folds)
    finally:
        lib.cvm_debug_resident(2)
    assert torch.equal(bx, fx) and torch.equal(by, fy)
    assert not torch.equal(bx, tx)                                       # (a different kernel: different roundings)
    scale = float(tx.abs().max())
    assert float((bx - tx).abs().max()) <= 1e-3 * scale                  # (sanity; the gate against the oracle is below)
    assert torch.equal(by, ty)                                           # (XTY: the tile kernel's arithmetic in res_pack_kernel)
    o = OracleCVMatrix()
    o.fit(X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64))
    o32 = OracleCVMatrix(dtype=np.float32)
    o32.fit(X, Y, w)
    for f in (0, 17, P - 1):
        (rx, ry), _ = o.training_XTX_XTY(folds[f])
        (sx, sy), _ = o32.training_XTX_XTY(folds[f])
        assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX")
        assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY")
        assert bool((bx[f] == bx[f].T).all())


@pytest.mark.parametrize("tool,args,env", [("fuzz_all.py", ["300", "101"], {}), ("fuzz_small.py", ["500", "102"], {}),
                                           ("fuzz_small.py", ["250", "103"], {"CVM_SMALL_MAXN": "128"}),
                                           ("fuzz_all.py", ["60", "104"], {"CVM_FUZZ_HARD": "1"}),
                                           ("fuzz_small.py", ["60", "105"], {"CVM_FUZZ_HARD": "1"})])
def test_randomised_routes_against_the_oracle(tool, args, env):
    """tools/fuzz_all.py / fuzz_small.py: random shapes, fold structures, element types, flags,
    weights, ddof, lazy or eager fit and call styles through every route of the fold stage,
    against the oracle (float64 1e-10; float32 twice the oracle's own float32 error + two roundings, cvmatrix_amd/fp32_gate.py).
    CVM_FUZZ_HARD=1: each case with one non-finite or overflowing cell, through the mask-aware comparison of hard_input_cases.py."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", tool), *args], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def torch_equal(x, y):
    import torch
    return bool(torch.equal(x, y))


def test_lazy_fit_other_first_uses_take_the_fit_kernel(amd):
    rng = np.random.default_rng(78)
    N, K, M = 3000, 40, 3
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    eg = amd.CVMatrix(lazy_fit=False)
    eg.fit(X, Y, w)
    sub = [np.arange(0, 500), np.arange(700, 1500)]              # not a partition
    for first_use in ("attribute", "per_fold", "subset", "statistics"):
        lz = amd.CVMatrix(lazy_fit=True)
        lz.fit(X, Y, w)
        assert lz._pending
        if first_use == "attribute":
            assert torch_equal(lz.XTX, eg.XTX) and torch_equal(lz.sum_X, eg.sum_X)
        elif first_use == "per_fold":
            (a, b), _ = lz.training_XTX_XTY(sub[0])
            (c, d), _ = eg.training_XTX_XTY(sub[0])
            assert torch_equal(a, c) and torch_equal(b, d)
        elif first_use == "subset":
            (a, b), _ = lz.training_XTX_XTY_batched(sub)
            (c, d), _ = eg.training_XTX_XTY_batched(sub)
            assert torch_equal(a, c) and torch_equal(b, d)
        else:
            sa = lz.training_statistics_batched(sub)
            sc = eg.training_statistics_batched(sub)
            assert all(torch_equal(s, t) for s, t in zip(sa, sc))
        assert not lz._pending and lz._sweep is None
        assert torch_equal(lz.XTY, eg.XTY)


def test_negative_device_weights_raise_in_fit_or_at_the_first_hand_out(amd):
    """cvmatrix.py:1188-1189 for weights that live on the device.  ``validate_weights="sync"``: fit() reads them back
    and raises itself.  Default (``"deferred"``): fit() counts the negative weights on the device and returns without
    waiting; every way of getting a result or an attribute of that fit raises -- lazy or eager fit, flags that need
    no statistics included (the reference raises whatever the flags are)."""
    import torch
    rng = np.random.default_rng(79)
    X = torch.from_numpy(rng.random((200, 8))).cuda()
    Y = torch.from_numpy(rng.random((200, 2))).cuda()
    w = torch.from_numpy(rng.random(200)).cuda()
    w[5] = -1.0
    msg = "Weights must be non-negative."
    for lazy in (True, False):
        with pytest.raises(ValueError, match=msg):
            amd.CVMatrix(lazy_fit=lazy, validate_weights="sync").fit(X, None, w)
        uses = [lambda m: m.training_XTX(np.arange(40)), lambda m: m.training_XTX_XTY(np.arange(3)),
                lambda m: m.training_XTX_XTY_batched(amd.Partitioner(np.arange(200) % 4)),
                lambda m: m.training_statistics(np.arange(40)), lambda m: m.XTX, lambda m: m.XTY, lambda m: m.sum_X,
                lambda m: m.num_nonzero_w, lambda m: m.sum_w,
                lambda m: [m.training_XTX_XTY(v) for v in amd.Partitioner(np.arange(200)).folds_dict.values()]]
        for flags in ((True,) * 4, (False,) * 4):
            for iu, use in enumerate(uses):
                m = amd.CVMatrix(*flags, lazy_fit=lazy, validate_weights="deferred")
                m.fit(X, Y, w)                                         # returns: nothing has been read back
                if flags[0] is False and 6 <= iu <= 8:
                    continue                                           # (those attributes are None without flags)
                for again in (0, 1):                                   # ... and keeps raising
                    try:
                        use(m)
                    except ValueError as e:
                        assert msg in str(e)
                    else:
                        raise AssertionError(f"use {iu} (flags {flags[0]}, lazy {lazy}, attempt {again}) did not raise")
    # host arrays are always checked inside fit(), before anything is uploaded
    with pytest.raises(ValueError, match=msg):
        amd.CVMatrix().fit(X.cpu().numpy(), None, w.cpu().numpy())


def test_deferred_weight_validation_counts_folds_only_where_the_bound_does_not_decide(amd):
    """Weights validated on the device: per-fold counts of non-zero weights are not taken while "a fold holds at most
    as many non-zero weights as rows" already rules both raises out (cvmatrix.py:612-630, 1074-1078); where it does
    not, they are counted exactly and the reference's raises come in the reference's order -- same verdicts as with
    host weights."""
    import torch
    rng = np.random.default_rng(80)
    N, K = 300, 6
    Xh, wh = rng.random((N, K)), rng.random(N) + 0.1
    p = amd.Partitioner(np.arange(N) % 3)
    # plenty of non-zero weights: nothing is counted, nothing is read back
    m = amd.CVMatrix(validate_weights="deferred")
    m.fit(torch.from_numpy(Xh).cuda(), None, torch.from_numpy(wh).cuda())
    b = m.prepare_folds(p)
    m.training_XTX_batched(b)
    assert not b.nz_known and m._w_host is None and m._w_verified and m.num_nonzero_w == N
    # only rows of fold 0 carry weight: training sets of folds 1, 2 are fine, fold 0's is empty
    wz = np.where(np.arange(N) % 3 == 0, wh, 0.0)
    ref = amd.CVMatrix()
    ref.fit(Xh, None, wz)
    for folds, msg in (([p.folds_dict[0]], "must be greater than zero"), ([p.folds_dict[1]], None)):
        m = amd.CVMatrix(validate_weights="deferred")
        m.fit(torch.from_numpy(Xh).cuda(), None, torch.from_numpy(wz).cuda())
        if msg:
            with pytest.raises(ValueError, match=msg):
                m.training_XTX_batched(folds)
            with pytest.raises(ValueError, match=msg):
                ref.training_XTX_batched(folds)
        else:
            got, want = m.training_XTX_batched(folds), ref.training_XTX_batched(folds)
            assert torch_equal(got[0], want[0])
    # exactly ddof + 0 non-zero weights left for training -> the ddof raise
    w1 = np.zeros(N); w1[0] = 1.0; w1[1] = 2.0
    m = amd.CVMatrix(ddof=1, validate_weights="deferred")
    m.fit(torch.from_numpy(Xh).cuda(), None, torch.from_numpy(w1).cuda())
    with pytest.raises(ValueError, match="must be greater than `ddof`"):
        m.training_XTX(np.array([1, 5, 7]))


def test_one_small_fold_per_call_sends_indices_with_the_launch(amd):
    """The reference's call pattern with tiny folds (leave-one-out): the indices of the single fold
    travel in the kernel arguments (CVM_IDX_HOST), no device index array is made; same XTX bits and
    statistics as the same fold inside a batch that uploads its indices."""
    import ctypes as C

    import torch
    from cvmatrix_amd import _lib
    rng = np.random.default_rng(31)
    N, K, M = 400, 70, 3
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    m = amd.CVMatrix(lazy_fit=False)
    m.fit(X, Y, w)
    for v in (np.array([7]), np.array([3, 3, -1, 250]), np.arange(100, 132)):
        b1 = m.prepare_folds([v])
        assert b1.inline
        (a, b), sa = m.training_XTX_XTY_batched(b1)
        assert b1.inline                                   # still no device copy
        b2 = m.prepare_folds([v, np.array([0, 1])])
        assert not b2.inline
        (c, d), sc = m.training_XTX_XTY_batched(b2)
        assert torch.equal(a[0], c[0])
        if v.size < 8:
            assert torch.equal(b[0], d[0])
        else:
            # (a batch of folds of eight rows or more takes mid_tile_kernel, whose XTY sums run on the matrix
            #  cores like its XTX sums; the one-fold call keeps the small-fold kernels' scalar XTY sums)
            assert float((b[0] - d[0]).norm() / d[0].norm()) < 1e-13
        for s, t in zip(sa, sc):
            assert torch.equal(s[0], t[0])
        st = m.training_statistics_batched(b1)             # statistics-only: uploads on demand
        assert not b1.inline and torch.equal(st[0][0], sc[0][0])
    # the flag is refused for anything but one small fold
    lib = _lib.load()
    off = np.array([0, 1, 2], dtype=np.int64)
    idx = np.array([1, 2], dtype=np.int64)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.empty((2, K, K), dtype=torch.float64, device="cuda")
    st4 = torch.empty((2, 4), dtype=torch.float64, device="cuda")
    mu = torch.empty((2, K), dtype=torch.float64, device="cuda")
    rc = lib.cvm_fold_update(m.X.data_ptr(), 0, 0, idx.ctypes.data, off.ctypes.data, off.ctypes.data, 2, N, K, 0,
                             _lib.CVM_F64, _lib.RET_XTX | _lib.IDX_HOST, 1.0, 1e-14, m.XTX.data_ptr(), 0,
                             m._gstats.data_ptr(), out.data_ptr(), 0, mu.data_ptr(), mu.data_ptr(), 0, 0,
                             st4.data_ptr(), ws.data_ptr(), ws.numel(), 0)
    assert rc == _lib.CVM_EINVAL and b"CVM_IDX_HOST" in lib.cvm_last_error()


@pytest.mark.parametrize("dtype,K", [(np.float64, 300), (np.float64, 500), (np.float32, 600), (np.float64, 100),
                                      (np.float64, 200), (np.float32, 500), (np.float32, 200)])
def test_leave_one_out_rows_kernel(amd, dtype, K):
    """One- and two-row folds of a matrix whose rows are not whole cache lines go through
    small_rows_kernel (whole output rows, both triangles computed): against the oracle, exactly
    symmetric, same bits with and without XTY."""
    rng = np.random.default_rng(K)
    N, M = 1500, 3
    X, Y = rng.random((N, K)).astype(dtype), rng.random((N, M)).astype(dtype)
    w = rng.random(N).astype(dtype)
    w[::11] = 0
    folds = [np.array([i]) for i in range(40)] + [np.array([100 + 2 * i, 101 + 2 * i]) for i in range(20)]
    f32 = dtype is np.float32
    for flags, ww in (((True,) * 4, w), ((False,) * 4, None), ((True, False, True, False), w)):
        m = amd.CVMatrix(*flags, dtype=dtype)
        m.fit(X, Y, ww)
        (bx, by), bst = m.training_XTX_XTY_batched(folds)
        o = OracleCVMatrix(*flags, dtype=np.float64)
        o.fit(X.astype(np.float64), Y.astype(np.float64), None if ww is None else ww.astype(np.float64))
        if f32:
            o32 = OracleCVMatrix(*flags, dtype=np.float32)      # the reference's own float32 arithmetic
            o32.fit(X, Y, ww)
        for f in (0, 13, 39, 40, 59):
            (rx, ry), rst = o.training_XTX_XTY(folds[f])
            if f32:
                (sx, sy), _ = o32.training_XTX_XTY(folds[f])
                assert_fp32_like_reference(bx[f], rx, sx, f"fold{f} XTX", floor=FP32_FLOOR)
                assert_fp32_like_reference(by[f], ry, sy, f"fold{f} XTY", floor=FP32_FLOOR)
            else:
                assert_normwise(bx[f].double(), rx, TOL, f"fold{f} XTX")
                assert_normwise(by[f].double(), ry, TOL, f"fold{f} XTY")
            assert bool((bx[f] == bx[f].T).all())
        bx1 = m.training_XTX_batched(folds)[0]
        assert bool((bx1 == bx).all())


@pytest.mark.parametrize("N,K,M,P,flags", [(30000, 260, 40, 200, (True,) * 4), (20000, 132, 66, 100, (True, False, True, False)),
                                           (24000, 516, 34, 60, (False,) * 4)])
def test_mid_size_folds_with_wide_y(amd, N, K, M, P, flags):
    """One unit per fold with more than 32 responses: the fused route has Y-chunk items next to the
    G tiles (all eight waves share the epilogue of a G tile, none that of a Y chunk)."""
    rng = np.random.default_rng(N + K)
    X, Y, w = rng.random((N, K)), rng.random((N, M)), rng.random(N)
    folds = [np.arange(i, N, P) for i in range(P)]
    m = amd.CVMatrix(*flags, lazy_fit=False)
    m.fit(X, Y, w)
    o = OracleCVMatrix(*flags)
    o.fit(X, Y, w)
    (bx, by), bst = m.training_XTX_XTY_batched(folds)
    bx1, _ = m.training_XTX_batched(folds)
    for f in (0, P // 2, P - 1):
        (rx, ry), rst = o.training_XTX_XTY(folds[f])
        assert_normwise(bx[f], rx, TOL, "XTX")
        assert_normwise(by[f], ry, TOL, "XTY")
        assert_normwise(bx1[f], rx, TOL, "XTX only")
        assert_stats(tuple(None if s is None else s[f] for s in bst), rst, TOL)
        assert bool((bx[f] == bx[f].T).all())
