"""Fixture generators and the accuracy gate of the device-ridge tests (tests/test_gpu_ridge.py on the
GPU; tests/test_ridge_oracle.py checks on the CPU that every generator meets its own conditions).
NumPy and the oracle only: nothing here touches the product."""

import os

import numpy as np

from oracle import ridge_oracle as ro

U = ro.U

K_VALUES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 255, 256, 257)
M_VALUES = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)

# (K, M): every K, every M, and (K + M) % 32 in {0, 1, 31} with K % 32 zero and non-zero
GRID = [(1, 1), (1, 31), (1, 32), (1, 64), (2, 2), (2, 31), (2, 63),
        (15, 16), (15, 17), (15, 48), (15, 49), (16, 15), (16, 16), (16, 17), (16, 47), (16, 49),
        (17, 15), (17, 16), (17, 47), (17, 48), (31, 1), (31, 32), (31, 33), (31, 64),
        (32, 1), (32, 31), (32, 32), (32, 64), (33, 31), (33, 32), (33, 64),
        (63, 1), (63, 2), (63, 33), (63, 64), (64, 17), (64, 31), (64, 33), (64, 64),
        (65, 32), (65, 48), (65, 63), (96, 1), (96, 32), (96, 49), (96, 63),
        (127, 1), (127, 32), (127, 64), (128, 31), (128, 33), (128, 64), (129, 15), (129, 63), (129, 64),
        (160, 32), (160, 33), (160, 63), (255, 1), (255, 47), (255, 64), (256, 1), (256, 33), (256, 63), (256, 64),
        (257, 2), (257, 32), (257, 63)]
# float32: 16 of them, one to four 16-wide tiles of responses, the three (K + M) % 32 classes
GRID_F32 = [(1, 1), (2, 31), (15, 17), (16, 15), (17, 48), (31, 33), (32, 31), (33, 64), (63, 64), (64, 64),
            (65, 32), (96, 63), (129, 64), (255, 64), (256, 33), (257, 63)]

LADDER_KM = [(33, 3), (33, 40), (96, 3), (96, 40), (257, 3), (257, 40)]
LADDER_COND = (1e4, 1e8, 1e10, 1e12)
LADDER_COND_F32 = (1e4, 1e6)

INFO_K = (33, 64, 70, 100)
INFO_PIVOTS = (1, 2, 32, 33, 34, 64, 65)           # and K itself


def ladder_lambdas(cond):
    """lam = 0, then penalties that bring cond(XTX + lam I) = (1 + lam) / (1 / cond + lam) down by decades."""
    return np.array([0.0, 10.0 / cond, 100.0 / cond, 1e4 / cond])


def info_pivots(K):
    return sorted({j for j in INFO_PIVOTS if j <= K} | {K})


def spd_spectrum(rng, F, K, M, cond, dtype=np.float64):
    """F distinct SPD matrices with singular values logspace(0, -log10(cond), K) under a random orthogonal
    Q each, symmetrised, and standard normal right-hand sides.  float32: rounded from these (symmetric
    still; the tests widen them again, which is exact)."""
    XTX = np.empty((F, K, K))
    s = np.logspace(0.0, -np.log10(cond), K)
    for f in range(F):
        Q, _ = np.linalg.qr(rng.standard_normal((K, K)))
        A = (Q * s) @ Q.T
        XTX[f] = 0.5 * (A + A.T)
    XTY = rng.standard_normal((F, K, M))
    return XTX.astype(dtype), XTY.astype(dtype)


def make_indefinite(A, j, depth=0.1):
    """Lower A[j][j] (j 1-based; A in place, any float dtype) so that the j-th Cholesky pivot becomes
    -depth ||A||_2: the first j - 1 pivots do not see the change."""
    A64 = A.astype(np.float64)
    info, piv = ro.cholesky_pivots(A64[:j, :j])
    assert info == 0, "make_indefinite wants a positive definite matrix"
    A[j - 1, j - 1] = A64[j - 1, j - 1] - piv[j - 1] - depth * np.linalg.norm(A64, 2)
    return A


def indefinite_fixture(K, j, dtype=np.float64, M=3):
    """Test (d): four well-conditioned folds, fold 1 indefinite at pivot j."""
    rng = np.random.default_rng(1000 * K + j)
    XTX, XTY = spd_spectrum(rng, 4, K, M, 1e2, dtype)
    make_indefinite(XTX[1], j)
    return XTX, XTY


def info_is_unambiguous(A, info, pivot, n2=None):
    """The oracle's call can be held against the kernel's: a failing pivot below -1e-3 ||A||_2, or no
    failure and every pivot above 1e3 K u ||A||_2 (`n2`: that norm, where the caller has it)."""
    if n2 is None:
        n2 = np.linalg.norm(np.asarray(A, dtype=np.float64), 2)
    if info:
        return bool(pivot < -1e-3 * n2)
    return bool(pivot > 1e3 * A.shape[0] * U * n2)


# ---- the gate (BASELINE.md section 4 / cvmatrix_amd/fp32_gate.py: twice the reference arithmetic's own
# error plus a few roundings; the yardstick comes from the reference side alone)

def references(XTX, XTY, lam):
    """ref (F, L, K, M) by ridge_solve_ref and Y (L,): per penalty the largest yardstick over the folds.
    float32 inputs are widened first (exact)."""
    XTX = np.asarray(XTX, dtype=np.float64)
    XTY = np.asarray(XTY, dtype=np.float64)
    F, K, M = XTY.shape
    ref = np.empty((F, len(lam), K, M))
    Y = np.zeros(len(lam))
    for f in range(F):
        for l, lv in enumerate(lam):
            ref[f, l] = ro.ridge_solve_ref(XTX[f], XTY[f], lv)
            Y[l] = max(Y[l], ro.yardstick(XTX[f], XTY[f], lv, ref[f, l]))
    return ref, Y


def gate_bound(Y, float32=False, factor=2.0):
    return (2.0 ** -24 if float32 else 0.0) + factor * Y + 4 * U


def assert_gate(B, ref, Y, what, float32=False, factor=2.0):
    """err(f, l) <= 2 Y(l) + 4 u (float32: plus the one float32 rounding of the store) for every problem
    of the batch; returns the largest err / Y.  CVM_RIDGE_REPORT=path: one line per comparison."""
    B = np.asarray(B, dtype=np.float64)
    report = os.environ.get("CVM_RIDGE_REPORT")
    lines, bad, worst = [], [], 0.0
    for f in range(ref.shape[0]):
        for l in range(ref.shape[1]):
            err = ro.rel_err(B[f, l], ref[f, l])
            worst = max(worst, err / Y[l] if Y[l] > 0 else 0.0)
            lines.append(f"{what} f={f} l={l}\t{err:.3e}\t{Y[l]:.3e}\n")
            if not err <= gate_bound(Y[l], float32, factor):
                bad.append((f, l, err, Y[l]))
    if report:
        with open(report, "a") as fh:
            fh.writelines(lines)
    assert not bad, f"{what}: error above {factor} x yardstick + 4u" + (" + 2^-24" if float32 else "") + \
        "; (fold, penalty, err, Y): " + ", ".join(f"({f}, {l}, {e:.3e}, {y:.3e})" for f, l, e, y in bad[:6])
    return worst


# ---- seeded random cases (test (j))

RANDOM_SEED = 20240607
RANDOM_DRAWS = 150


def random_draws(seed=RANDOM_SEED, n=RANDOM_DRAWS):
    """n draws of a batch: K in 1..300, M in 1..64, F in 3..6, L in 1..8, dtype, cond in 1e1..1e10
    (float32: to 1e6, as the float32 ladder, so that rounding the matrix to float32 leaves it positive definite), penalties
    log-uniform in 1e-8..1e2, and in one draw in ten one fold made indefinite at a random pivot."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        K = int(rng.integers(1, 301))
        M = int(rng.integers(1, 65))
        F = int(rng.integers(3, 7))
        L = int(rng.integers(1, 9))
        dtype = np.float32 if rng.random() < 0.3 else np.float64
        cond = 10.0 ** rng.uniform(1.0, 6.0 if dtype == np.float32 else 10.0)
        lam = 10.0 ** rng.uniform(-8.0, 2.0, L)
        XTX, XTY = spd_spectrum(rng, F, K, M, cond, dtype)
        bad_fold = None
        if i % 10 == 7:
            bad_fold = int(rng.integers(0, F))
            make_indefinite(XTX[bad_fold], int(rng.integers(1, K + 1)), depth=200.0)    # below every penalty
        yield dict(i=i, K=K, M=M, F=F, L=L, dtype=dtype, cond=cond, lam=lam, XTX=XTX, XTY=XTY, bad_fold=bad_fold)


def oracle_info(XTX, lam):
    """(info (F, L) int, callable (F, L) bool) from cholesky_info on XTX[f] + lam[l] I in float64."""
    XTX = np.asarray(XTX, dtype=np.float64)
    F, K = XTX.shape[:2]
    info = np.zeros((F, len(lam)), dtype=np.int64)
    sure = np.zeros((F, len(lam)), dtype=bool)
    for f in range(F):
        finite = np.all(np.isfinite(XTX[f]))
        ev = np.linalg.eigvalsh(XTX[f]) if finite else None      # symmetric: ||XTX + lam I||_2 = max |ev + lam|
        for l, lv in enumerate(lam):
            A = XTX[f] + lv * np.eye(K)
            info[f, l], p = ro.cholesky_info(A)
            sure[f, l] = info_is_unambiguous(A, info[f, l], p, np.abs(ev + lv).max() if finite else None)
    return info, sure
