"""The reference and the gate of the validation scorer's tests (tests/test_sse_host.py on the CPU,
tests/test_gpu_sse.py on the device), an emulation of the scorer's arithmetic with five deliberate mistakes, and
the designs the tests share.  The products are cv_predict's (one main loop): what predict_cases.py derives for
them is taken from there.

REFERENCE.  For one fold with rows i, model a and response m, in np.longdouble (63 mantissa bits where this
suite runs: predict_cases.require_longdouble skips elsewhere) from the arrays the device actually read -- for
float32 the float32 values, widened exactly:
    z = (x_i - muX) / sdX        p = z . B[a][:, m]        S = |z| . |B[a][:, m]|
    e_i = p sdY[m] + muY[m] - y_im
    sse_ref[a][m] = sum_i w_i e_i^2        wsum_ref = sum_i w_i
An absent statistic is 0 / 1, absent weights are 1.

GATE, derived and not calibrated.  With u = 2^-53 (float64) or 2^-24 (float32) the error the kernel may make in
e_i is bounded by
    g_i = 2 (K + 8) u S |sdY| + 3 2^-53 (|p sdY| + |muY| + |y|)
The first term is predict_cases' own: one rounding of z to the dtype, four float64 roundings in forming it, K
accumulations in the dtype, with a factor 2 for a matrix core whose inner sum of four products need not be
round-to-nearest.  predict_cases' last term is the rounding of the prediction to the dtype, which the scorer
does not make: the accumulator is widened exactly and the epilogue is three float64 operations -- the product
with sdY, the sum with muY, the difference with y -- each rounding a number no larger than |p sdY| + |muY| + |y|.
An error d_i, |d_i| <= g_i, moves w_i e_i^2 by w_i |2 e_i d_i + d_i^2|; the square, the product with the weight
and a float64 sum of at most n terms (in whatever order) each round numbers no larger than sum w (|e| + g)^2:
    |sse - sse_ref|   <= sum_i w_i (2 |e_i| g_i + g_i^2) + (n + 4) 2^-53 sum_i w_i (|e_i| + g_i)^2
    |wsum - wsum_ref| <= n 2^-53 sum_i |w_i|,     and wsum == n exactly where there are no weights
(integers up to 2^53 add exactly).  Where a bound is 0 -- an empty fold, a fold whose weights are all 0 -- the
result must BE the reference.  A sequential emulation of the kernel (`emulate`) lands well inside and each of
its five mutants outside (tests/test_sse_host.py prints where).  A result over the gate is a finding about the
kernel, not a reason to widen the gate."""

import numpy as np

import predict_cases as pc

LD = pc.LD
U64 = LD(2.0 ** -53)
MUTANTS = ("dropped_row", "neighbour_response", "weights_by_position", "no_k_tail", "coarse_reciprocal")
SIZES = (1, 63, 0, 64, 65, 129)


def _wide(a, width, fill):
    return np.full(width, fill, dtype=LD) if a is None else np.asarray(a).astype(LD)


def reference(X, Y, w, rows, B, stats=None):
    """One fold.  X (N, K), Y (N, M), w (N,) or None, rows the fold's row numbers, B (A, K, M), stats None or
    (muX, sdX, muY, sdY) of 1-D arrays / None.  Returns (sse_ref, gate) (A, M) and (wsum_ref, wgate) scalars, all
    np.longdouble; the unit of the gate is that of X's dtype."""
    muX, sdX, muY, sdY = stats if stats is not None else (None,) * 4
    rows = np.asarray(rows, dtype=np.int64)
    n, K = rows.size, X.shape[1]
    A, _, M = np.asarray(B).shape
    u = LD(pc.unit(X.dtype))
    Z = (X[rows].astype(LD) - _wide(muX, K, 0)) / _wide(sdX, K, 1)
    flat = np.asarray(B).astype(LD).transpose(1, 0, 2).reshape(K, A * M)
    p = (Z @ flat).reshape(n, A, M)
    S = (np.abs(Z) @ np.abs(flat)).reshape(n, A, M)
    sy, my = _wide(sdY, M, 1), _wide(muY, M, 0)
    y = Y[rows].astype(LD)[:, None, :]
    wv = np.ones(n, dtype=LD) if w is None else np.asarray(w)[rows].astype(LD)
    e = p * sy + my - y
    g = 2 * (K + 8) * u * S * np.abs(sy) + 3 * U64 * (np.abs(p * sy) + np.abs(my) + np.abs(y))
    wa = np.abs(wv)[:, None, None]
    sse = (wv[:, None, None] * e * e).sum(axis=0)
    gate = (wa * (2 * np.abs(e) * g + g * g)).sum(axis=0) + (n + 4) * U64 * (wa * (np.abs(e) + g) ** 2).sum(axis=0)
    return sse, gate, wv.sum(), n * U64 * np.abs(wv).sum()


def cv_reference(X, Y, w, folds, B, stats):
    """Every fold of a batch: folds a list of index arrays, B (F, A, K, M), stats a 4-tuple of (F, width) arrays
    / None.  Returns sse_ref, gate (F, A, M) and wsum_ref, wgate (F,)."""
    out = [reference(X, Y, w, v, B[f], pc.fold_stats(stats, f)) for f, v in enumerate(folds)]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def one_row_fold_reference(Xr, y, w, B, stats):
    """Folds of one row each, all at once (A = M = 1): Xr (F, K) the folds' rows, y and w (F,) their responses
    and weights, B (F, 1, K, 1), stats (F, K) / (F, 1) arrays (all present).  Returns what `reference` returns,
    each (F,) -- sse_ref and gate as (F, 1, 1)."""
    muX, sdX, muY, sdY = (np.asarray(s).astype(LD) for s in stats)
    F, K = Xr.shape
    u = LD(pc.unit(Xr.dtype))
    Z = (Xr.astype(LD) - muX) / sdX
    b = np.asarray(B)[:, 0, :, 0].astype(LD)
    p, S = (Z * b).sum(axis=1), (np.abs(Z) * np.abs(b)).sum(axis=1)
    sy, my, yl, wl = sdY[:, 0], muY[:, 0], np.asarray(y).astype(LD), np.asarray(w).astype(LD)
    e = p * sy + my - yl
    g = 2 * (K + 8) * u * S * np.abs(sy) + 3 * U64 * (np.abs(p * sy) + np.abs(my) + np.abs(yl))
    wa = np.abs(wl)
    gate = wa * (2 * np.abs(e) * g + g * g) + (1 + 4) * U64 * wa * (np.abs(e) + g) ** 2
    return (wl * e * e).reshape(F, 1, 1), gate.reshape(F, 1, 1), wl, U64 * wa


def worst_ratio(sse, ref, gate):
    """The largest |sse - ref| / gate; where the gate is zero the result must be the reference itself."""
    sse = np.asarray(sse)
    assert sse.shape == ref.shape and sse.dtype == np.float64, (sse.shape, ref.shape, sse.dtype)
    if sse.size == 0:
        return 0.0
    assert np.isfinite(sse).all(), "non-finite errors from finite inputs"
    d = np.abs(sse.astype(LD) - ref)
    zero = gate == 0
    assert (d[zero] == 0).all(), "a sum with a zero gate differs from the reference"
    return float((d[~zero] / gate[~zero]).max()) if (~zero).any() else 0.0


def assert_gate(sse, wsum, refs, what="", weighted=True):
    """sse (..., A, M) and wsum (...) against `refs` = (sse_ref, gate, wsum_ref, wgate): every column of every
    fold.  Prints and returns the largest fraction of the sse gate."""
    sse_ref, gate, wsum_ref, wgate = refs
    worst = worst_ratio(sse, sse_ref, gate)
    print(f"{what}: {worst:.4f} of the gate")
    assert worst <= 1.0, f"{what}: {worst:.4f} of the gate"
    wsum = np.asarray(wsum)
    assert wsum.dtype == np.float64 and wsum.shape == np.shape(wsum_ref)
    if weighted:
        assert (np.abs(wsum.astype(LD) - wsum_ref) <= wgate).all(), f"{what}: wsum"
    else:
        assert (wsum.astype(LD) == wsum_ref).all(), f"{what}: wsum is not the row count"
    return worst


def emulate(X, Y, w, rows, B, stats=None, mutant=None):
    """The scorer's arithmetic for one fold, step by step in NumPy: predict_cases.emulate up to the accumulator
    (z formed in float64 and rounded to the dtype, one accumulator per column summed over k in order in the
    dtype), the epilogue in float64 (times sdY, plus muY, minus y; the square; times the weight), the rows summed
    in order.  Returns (sse (A, M) float64, wsum float64).  `mutant`: one of MUTANTS --
      dropped_row           the fold's last row is left out
      neighbour_response    muY / sdY of response m + 1 (cyclically)
      weights_by_position   w[i] of the row's position in the fold, not w[rows[i]]
      no_k_tail             the k past the last whole stage of 16 are left out
      coarse_reciprocal     1 / sdX good to 2^-24 only (rounded to float32)"""
    assert mutant is None or mutant in MUTANTS, mutant
    muX, sdX, muY, sdY = stats if stats is not None else (None,) * 4
    rows = np.asarray(rows, dtype=np.int64)
    n, K = rows.size, X.shape[1]
    A, _, M = B.shape
    Kk = K // 16 * 16 if mutant == "no_k_tail" else K
    if mutant == "coarse_reciprocal" and sdX is not None:
        # (a standard deviation whose float64 reciprocal is the float32-rounded one, to the last place)
        # (predict_cases.emulate reads the statistics in float64 and takes them as they are)
        sdX = 1.0 / (1.0 / np.asarray(sdX, dtype=np.float64)).astype(np.float32).astype(np.float64)

    def cut(s):
        return None if s is None else np.asarray(s)[:Kk]

    Xr = np.ascontiguousarray(X[rows][:, :Kk])
    acc = pc.emulate(Xr, np.asarray(B)[:, :Kk], (cut(muX), cut(sdX), None, None))
    assert acc.dtype == X.dtype
    sy = np.ones(M) if sdY is None else np.asarray(sdY, dtype=np.float64)
    my = np.zeros(M) if muY is None else np.asarray(muY, dtype=np.float64)
    if mutant == "neighbour_response":
        sy, my = np.roll(sy, -1), np.roll(my, -1)
    if w is None:
        wv = np.ones(n)
    elif mutant == "weights_by_position":
        wv = np.asarray(w, dtype=np.float64)[:n]
    else:
        wv = np.asarray(w, dtype=np.float64)[rows]
    y = Y[rows].astype(np.float64)
    last = n - 1 if mutant == "dropped_row" else n
    sse, wsum = np.zeros((A, M)), np.float64(0.0)
    for i in range(last):
        e = acc[i].astype(np.float64) * sy + my - y[i]
        sse = sse + wv[i] * (e * e)
        wsum = wsum + wv[i]
    return sse, wsum


def design(rng, sizes, K, A, M, dtype, mask=(True, True, True, True), weighted=True, extra=0):
    """predict_cases.design and ragged_folds, plus Y and weights: rows with offsets and unequal column scales,
    coefficients of both signs, statistics near the data's own, responses of the predictions' size with an
    offset, weights in [0.2, 2).  Returns a dict: X (N, K), Y (N, M), w (N,) or None, folds, B (F, A, K, M),
    stats (a 4-tuple of (F, width) / None), all in `dtype`."""
    dt = np.dtype(dtype)
    folds, N = pc.ragged_folds(rng, sizes, extra)
    X, B, stats = pc.design(rng, N, K, A, M, dt, mask, F=len(sizes))
    Y = (rng.normal(size=(N, M)) * 3 + 1).astype(dt)
    w = rng.uniform(0.2, 2.0, N).astype(dt) if weighted else None
    return dict(X=X, Y=Y, w=w, folds=folds, B=B, stats=stats)


def hard_design(rng, sizes, K, A, M, dtype):
    """Values that are hard on the scorer.  The columns of X sit at 1e3 times their spread (the centring
    cancels three digits), every model fits nearly perfectly -- Y is the prediction of the fold's first model
    plus a residual of 1e-3 of the response's scale, the other models differ from the first by 1e-4 -- so the
    error e is a thousandth of the prediction p it is the difference of, muY is 1e4 times the residual, and a
    fifth of the weights are zero."""
    dt = np.dtype(dtype)
    folds, N = pc.ragged_folds(rng, sizes)
    F = len(sizes)
    spread = 10.0 ** rng.uniform(-1, 1, K)
    shift = 1e3 * spread * rng.choice([-1.0, 1.0], K)
    X = (rng.normal(size=(N, K)) * spread + shift).astype(dt)
    muX = (shift + 0.1 * spread * rng.normal(size=(F, K))).astype(dt)
    sdX = (spread * rng.uniform(0.8, 1.25, (F, K))).astype(dt)
    base = rng.normal(size=(F, 1, K, M)) / np.sqrt(K)
    B = (base + 1e-4 * rng.normal(size=(F, A, K, M)) / np.sqrt(K)).astype(dt)
    sdY = rng.uniform(0.5, 3.0, (F, M)).astype(dt)
    resid = 1e-3 * sdY.astype(np.float64)
    muY = (1e4 * resid * rng.choice([-1.0, 1.0], (F, M))).astype(dt)
    Y = np.zeros((N, M), dtype=dt)
    for f, v in enumerate(folds):
        Z = (X[v].astype(np.float64) - muX[f]) / sdX[f]
        Y[v] = (Z @ B[f, 0].astype(np.float64) * sdY[f] + muY[f] + resid[f] * rng.normal(size=(v.size, M))).astype(dt)
    w = rng.uniform(0.2, 2.0, N)
    w[rng.random(N) < 0.2] = 0.0
    return dict(X=X, Y=Y, w=w.astype(dt), folds=folds, B=B, stats=(muX, sdX, muY, sdY))
