"""The reference and the gate of the prediction tests (tests/test_predict_host.py on the CPU,
tests/test_gpu_predict.py on the device), and the designs they share.

REFERENCE.  out[r][a][m] = ((x - muX) / sdX) . B[a][:, m] * sdY[m] + muY[m], evaluated in np.longdouble (63
mantissa bits where this suite runs: `require_longdouble` skips elsewhere) from the arrays the device actually
read -- for float32 the float32 values, widened exactly.

GATE, per element, derived and not calibrated: with u = 2^-53 (float64) or 2^-24 (float32), Z the standardised
rows and S = |Z| @ |B[a]|,
    |out - ref| <= 2 (K + 8) u S |sdY| + 2 u |ref|
K + 8: one rounding of z to the dtype (u), at most 4 * 2^-53 in forming it (the subtraction, the reciprocal
within one unit, the product), K accumulations in the dtype, the float64 scale-and-shift; the factor 2 allows
the matrix core's inner sum of four products not to be round-to-nearest; 2 u |ref| is the one rounding of the
result to the dtype, with room for the reference's own 2^-64.  A sequential emulation of the kernel (`emulate`)
lands well inside (tests/test_predict_host.py prints where).  A result over the gate is a finding about the
kernel, not a reason to widen the gate."""

import numpy as np
import pytest

LD = np.longdouble
GRID_K = (1, 3, 4, 15, 16, 17, 33, 130)
# (A, M) with A M = 1, 9, 63, 64, 65 and one past the widest kernel variant (320 columns in float64, 384 in
# float32); odd M, M = 1 with A = 1, M at its limit of 64
GRID_AM = {"float64": ((1, 1), (3, 3), (9, 7), (1, 64), (4, 16), (13, 5), (107, 3)),
           "float32": ((1, 1), (3, 3), (9, 7), (1, 64), (4, 16), (13, 5), (55, 7))}
RAGGED = (1, 63, 64, 65, 129)


def require_longdouble():
    if np.finfo(LD).nmant < 63:
        pytest.skip("np.longdouble has fewer than 63 mantissa bits here: no reference")
    assert np.finfo(LD).nmant >= 63


def unit(dtype) -> float:
    return 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24


def reference(X, B, stats=None):
    """X (n, K), B (A, K, M), stats None or (muX, sdX, muY, sdY) of 1-D arrays / None.  Returns (ref, gate),
    both (n, A, M) np.longdouble; the unit of the gate is that of X's dtype."""
    muX, sdX, muY, sdY = stats if stats is not None else (None,) * 4
    n, K = X.shape
    u = LD(unit(X.dtype))
    Z = X.astype(LD)
    if muX is not None:
        Z = Z - np.asarray(muX).astype(LD)
    if sdX is not None:
        Z = Z / np.asarray(sdX).astype(LD)
    Bl = np.asarray(B).astype(LD)
    A, _, M = Bl.shape
    flat = Bl.transpose(1, 0, 2).reshape(K, A * M)
    ref = (Z @ flat).reshape(n, A, M)
    S = (np.abs(Z) @ np.abs(flat)).reshape(n, A, M)
    sy = np.ones(M, dtype=LD) if sdY is None else np.asarray(sdY).astype(LD)
    ref = ref * sy
    if muY is not None:
        ref = ref + np.asarray(muY).astype(LD)
    gate = 2 * (K + 8) * u * S * np.abs(sy) + 2 * u * np.abs(ref)
    return ref, gate


def fold_stats(stats, f):
    return tuple(None if s is None else np.asarray(s)[f] for s in stats)


def cv_reference(X, folds, B, stats):
    """order="folds": the folds' rows one after the other.  X (N, K), folds a list of index arrays, B
    (F, A, K, M), stats a 4-tuple of (F, width) arrays / None."""
    refs, gates = [], []
    for f, v in enumerate(folds):
        r, g = reference(X[v], B[f], fold_stats(stats, f))
        refs.append(r)
        gates.append(g)
    return np.concatenate(refs), np.concatenate(gates)


def worst_ratio(out, ref, gate):
    """The largest |out - ref| / gate; where the gate is zero (a prediction that is exactly zero) the result
    must be the reference itself."""
    out = np.asarray(out)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    if out.size == 0:
        return 0.0
    assert np.isfinite(out).all(), "non-finite predictions from finite inputs"
    d = np.abs(out.astype(LD) - ref)
    zero = gate == 0
    assert (d[zero] == 0).all(), "a prediction with a zero gate differs from the reference"
    return float((d[~zero] / gate[~zero]).max()) if (~zero).any() else 0.0


def assert_gate(out, ref, gate, what=""):
    w = worst_ratio(out, ref, gate)
    print(f"{what}: {w:.3f} of the gate")
    assert w <= 1.0, f"{what}: {w:.3f} of the gate"
    return w


def emulate(X, B, stats=None):
    """The kernel's arithmetic step by step in NumPy: z formed in float64 and rounded to the dtype, one
    accumulator per prediction summed over k in order in the dtype, the scale-and-shift in float64, one
    rounding to the dtype.  (Sequential: the matrix core sums four products at a time.)"""
    muX, sdX, muY, sdY = stats if stats is not None else (None,) * 4
    dt = X.dtype
    n, K = X.shape
    A, _, M = B.shape
    mu = np.zeros(K) if muX is None else np.asarray(muX, dtype=np.float64)
    isd = np.ones(K) if sdX is None else 1.0 / np.asarray(sdX, dtype=np.float64)
    Z = ((X.astype(np.float64) - mu) * isd).astype(dt)
    flat = np.ascontiguousarray(np.asarray(B, dtype=dt).transpose(1, 0, 2).reshape(K, A * M))
    acc = np.zeros((n, A * M), dtype=dt)
    for k in range(K):
        acc = (acc + (Z[:, k:k + 1] * flat[k:k + 1]).astype(dt)).astype(dt)
    sy = np.ones(M) if sdY is None else np.asarray(sdY, dtype=np.float64)
    my = np.zeros(M) if muY is None else np.asarray(muY, dtype=np.float64)
    return (acc.reshape(n, A, M).astype(np.float64) * sy + my).astype(dt)


def design(rng, n, K, A, M, dtype, mask=(True, True, True, True), F=None):
    """Rows with offsets and unequal column scales (what centring and scaling are for), coefficients of both
    signs, statistics near the data's own.  F None: one model, 1-D statistics; else F stacked ones."""
    dt = np.dtype(dtype)
    lead = () if F is None else (F,)
    scale = 10.0 ** rng.uniform(-1, 1, K)
    shift = rng.normal(size=K) * 3
    X = (rng.normal(size=(n, K)) * scale + shift).astype(dt)
    B = rng.normal(size=lead + (A, K, M)).astype(dt)
    full = ((shift + 0.1 * rng.normal(size=lead + (K,))).astype(dt),
            (scale * rng.uniform(0.8, 1.25, lead + (K,))).astype(dt),
            (rng.normal(size=lead + (M,)) * 2).astype(dt),
            rng.uniform(0.5, 3.0, lead + (M,)).astype(dt))
    stats = tuple(s if keep else None for s, keep in zip(full, mask))
    return X, B, stats


def ragged_folds(rng, sizes=RAGGED, extra=0):
    """Index arrays of the given sizes over a shuffled range(sum(sizes) + extra): `extra` rows in no fold."""
    N = int(sum(sizes)) + extra
    perm = rng.permutation(N).astype(np.int64)
    out, p = [], 0
    for s in sizes:
        out.append(perm[p:p + s].copy())
        p += s
    return out, N


def same_bits(a, b):
    """Bitwise equality, NaN payloads included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def one_row_fold_reference(Xr, B, stats):
    """Folds of one row each, all at once: Xr (F, K) the folds' rows, B (F, 1, K, 1), stats (F, K) / (F, 1)
    arrays (all present).  Returns (ref, gate), both (F,)."""
    muX, sdX, muY, sdY = (np.asarray(s).astype(LD) for s in stats)
    K = Xr.shape[1]
    u = LD(unit(Xr.dtype))
    Z = (Xr.astype(LD) - muX) / sdX
    b = np.asarray(B)[:, 0, :, 0].astype(LD)
    ref = (Z * b).sum(axis=1) * sdY[:, 0] + muY[:, 0]
    S = (np.abs(Z) * np.abs(b)).sum(axis=1)
    return ref, 2 * (K + 8) * u * S * np.abs(sdY[:, 0]) + 2 * u * np.abs(ref)
