"""Input builders and comparison helpers of the hard-input tests of the fold stage: non-finite cells, column
offsets that make the centring correction cancel, column and weight scales spread over many decades
(tests/test_gpu_hard_inputs.py on the GPU; tests/test_hard_inputs_oracle.py checks on the CPU that every
case meets its own conditions for the oracle alone).  NumPy and the oracle only: nothing here touches the
product."""

import os

import numpy as np

from cvmatrix_amd.fp32_gate import fp32_floor
from oracle.cvmatrix_oracle import OracleCVMatrix, naive_training_matrices

ON, OFF = (True,) * 4, (False,) * 4
CENTRE_ONLY = (True, True, False, False)
STAT_NAMES = ("muX", "sdX", "muY", "sdY")
NAMES = ("XTX", "XTY") + STAT_NAMES
X_KINDS = ("nan_x", "posinf_x", "infpair_x", "nan_x_zero_w")
KINDS = X_KINDS + ("nan_y", "nan_w", "overflow_x")
TOL64 = 1e-10
STAT_RTOL = {np.float64: 1e-10, np.float32: 2e-6}       # assert_stats's rule / the suite's F32_STAT_RTOL
TINY = float(np.finfo(np.float64).tiny)


# ---------------------------------------------------------------------------------------- one defect
def pair_row(row, N):
    """The row that takes the -Inf of an ``infpair_x`` defect."""
    return (row + 1) % N


def poisoned(X, Y, w, kind, row, col):
    """Copies of (X, Y, w) with one defect at (row, col); ``nan_y`` poisons column ``col % M`` of Y.  Y and w may be
    None where the kind does not touch them."""
    X, Y, w = X.copy(), None if Y is None else Y.copy(), None if w is None else w.copy()
    if kind == "nan_x":
        X[row, col] = np.nan
    elif kind == "posinf_x":
        X[row, col] = np.inf
    elif kind == "infpair_x":
        X[row, col] = np.inf
        X[pair_row(row, X.shape[0]), col] = -np.inf
    elif kind == "nan_x_zero_w":
        X[row, col] = np.nan
        w[row] = 0
    elif kind == "nan_y":
        Y[row, col % Y.shape[1]] = np.nan
    elif kind == "nan_w":
        w[row] = np.nan
    elif kind == "overflow_x":
        assert X.dtype == np.float64, "overflow_x is a float64 defect (finite; its square is not)"
        X[row, col] = 1e200
    else:
        raise ValueError(kind)
    return X, Y, w


def expected_masks(kind, flags, K, M, col, stats_only=False):
    """Where NumPy's arithmetic leaves a non-finite number, per output (None: the output is None under
    these flags).  ``stats_only``: the outputs of ``training_statistics``."""
    cX, cY, sX, sY = flags
    m = {"XTX": np.zeros((K, K), bool), "XTY": np.zeros((K, M), bool)}
    if stats_only:
        has = {"muX": cX or sX, "sdX": sX, "muY": cY or sY, "sdY": sY}
    else:
        has = {"muX": cX or cY, "sdX": sX, "muY": cX or cY, "sdY": sY}
    for n in STAT_NAMES:
        m[n] = np.zeros((1, K if n.endswith("X") else M), bool) if has[n] else None
    if kind in X_KINDS or (kind == "overflow_x" and any(flags)):
        m["XTX"][col, :] = m["XTX"][:, col] = True
        m["XTY"][col, :] = True
        for n in ("muX", "sdX"):
            if m[n] is not None and not (kind == "overflow_x" and n == "muX"):
                m[n][0, col] = True
    elif kind == "overflow_x":
        m["XTX"][col, col] = True
    elif kind == "nan_y":
        m["XTY"][:, col % M] = True
        for n in ("muY", "sdY"):
            if m[n] is not None:
                m[n][0, col % M] = True
    elif kind == "nan_w":
        for n in NAMES:
            if m[n] is not None:
                m[n][...] = True
    if stats_only:
        m["XTX"] = m["XTY"] = None
    return m


# ---------------------------------------------------------------------------------------- the gates
def gate_float64(tol=TOL64):
    """``assert_normwise``'s two conditions over the selected entries."""
    def gate(g, r, sel, what):
        d = g - r
        scale = max(np.abs(r).max(), TINY)
        assert np.abs(d).max() <= tol * scale, f"{what}: max|d|={np.abs(d).max():.3e} > {tol}*{scale:.3e}"
        assert np.linalg.norm(d) <= tol * max(np.linalg.norm(r), TINY), f"{what}: Frobenius"
    return gate


def gate_float32(ref32, floor=None):
    """``assert_fp32_like_reference``'s rule over the selected entries: ``ref32`` is the oracle's own float32
    run on the same float32 inputs."""
    floor = fp32_floor() if floor is None else floor
    ref32 = np.asarray(ref32, dtype=np.float64)

    def gate(g, r, sel, what):
        scale = max(np.abs(r).max(), TINY)
        err = np.abs(g - r).max() / scale
        yard = np.abs(ref32[sel] - r).max() / scale
        assert err <= 2 * yard + floor, f"{what}: error {err:.3e} > 2 x reference float32 error {yard:.3e} + {floor}"
    return gate


def gate_stats(rtol, atol=0, scale=None):
    """``assert_stats``'s rule: element-wise relative.  ``scale`` (an array like the statistic): each entry is held
    to ``rtol`` of the larger of itself and its scale (``mean_scales``)."""
    def gate(g, r, sel, what):
        bound = atol + rtol * (np.abs(r) if scale is None else np.maximum(np.abs(r), np.reshape(scale, sel.shape)[sel]))
        bad = np.flatnonzero(~(np.abs(g - r) <= bound))
        assert bad.size == 0, (f"{what}: {bad.size} entries beyond rtol {rtol}; first at {bad[0]}: {g[bad[0]]!r} against "
                               f"{r[bad[0]]!r}, |d| = {abs(g[bad[0]] - r[bad[0]]):.3e} > {bound[bad[0]]:.3e}")
    return gate


def mean_scales(X, Y, w, val):
    """The scale of a weighted mean's rounding error: sum(w |x|) / sum(w) over the training rows, per column of X and
    of Y.  A mean of signed values may be far below it (weights over six decades leave some twenty effective rows: in
    the float32 mid-tile spread case one column's mean is 1/800 of it, and the oracle's own float32 run is off by
    1.7e-5 of that mean, 6e-7 of this scale), and no summation in the element type can be held to a fraction of the
    mean there.  Where the values share a sign, as in the rest of the suite, it is |mean|.  Returns name -> array."""
    keep = np.ones(X.shape[0], bool)
    keep[np.asarray(val, dtype=int)] = False
    wd = np.ones(int(keep.sum())) if w is None else w[keep].astype(np.float64)
    return {"muX": (wd[:, None] * np.abs(X[keep].astype(np.float64))).sum(0) / wd.sum(),
            "muY": (wd[:, None] * np.abs(Y[keep].astype(np.float64))).sum(0) / wd.sum()}


def assert_matches_oracle_where_finite(got, ref, gate, what="", blocks=None):
    """The non-finite mask of ``got`` is the oracle's, element for element; the finite entries meet ``gate``
    with the scale taken over the finite entries of ``ref``.  ``blocks``: boolean masks that split the
    array into parts, each compared against its own scale."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad_g, bad_r = ~np.isfinite(got), ~np.isfinite(ref)
    if not np.array_equal(bad_g, bad_r):
        leak = np.argwhere(bad_g & ~bad_r)
        lost = np.argwhere(~bad_g & bad_r)
        raise AssertionError(f"{what}: non-finite mask differs from the oracle's: {len(leak)} entries non-finite only in "
                             f"the result (first {leak[:4].tolist()}), {len(lost)} finite only in the result "
                             f"(first {lost[:4].tolist()})")
    for b, blk in enumerate([np.ones(ref.shape, bool)] if blocks is None else blocks):
        sel = blk & ~bad_r
        if sel.any():
            gate(got[sel], ref[sel], sel, f"{what} block {b}" if blocks is not None else what)


def refuse_vacuous(kind, ref, K):
    """A comparison that cannot fail proves nothing: the reference must be poisoned somewhere, and (unless the
    weights are) must keep at least (K - 1)^2 entries of XTX finite.  ``ref``: name -> oracle array or None."""
    arrs = [np.asarray(v, dtype=np.float64) for v in ref.values() if v is not None]
    assert arrs and any((~np.isfinite(a)).any() for a in arrs), f"{kind}: the oracle has no non-finite entry"
    if kind != "nan_w" and ref.get("XTX") is not None:
        n = int(np.isfinite(ref["XTX"]).sum())
        assert n >= (K - 1) ** 2, f"{kind}: only {n} finite entries of XTX in the oracle"


def overflow_blocks(shape, col, rows_only=False):
    """Row and column ``col`` against their own max, the rest against its own: otherwise 1e200 hides the rest."""
    rc = np.zeros(shape, bool)
    rc[col, :] = True
    if not rows_only:
        rc[:, col] = True
    return [rc, ~rc]


def compare_fold(got, ref, ref32, kind, col, dtype, what=""):
    """One fold: the six outputs (name -> array or None) of the product against the float64 oracle's (``ref32``: the
    oracle's float32 run, float32 cases only)."""
    K = ref["XTX"].shape[0] if ref.get("XTX") is not None else None
    refuse_vacuous(kind, ref, K)
    for n in NAMES:
        r, g = ref.get(n), got.get(n)
        assert (g is None) == (r is None), f"{what}: None pattern differs at {n}"
        if r is None:
            continue
        w_ = f"{what} {n}"
        if n in STAT_NAMES:
            assert_matches_oracle_where_finite(np.reshape(g, np.shape(r)), r, gate_stats(STAT_RTOL[dtype]), w_)
            continue
        gate = gate_float64() if dtype is np.float64 else gate_float32(ref32[n])
        blocks = overflow_blocks(np.shape(r), col, rows_only=(n == "XTY")) if kind == "overflow_x" else None
        assert_matches_oracle_where_finite(g, r, gate, w_, blocks)
    if got.get("XTX") is not None:
        x = np.asarray(got["XTX"], dtype=np.float64)
        fin = np.isfinite(x)
        assert np.array_equal(fin, fin.T), f"{what}: the non-finite mask of XTX is not symmetric"
        assert np.array_equal(x[fin & fin.T], x.T[fin & fin.T]), f"{what}: XTX != XTX.T on finite entries"


def oracle_fold_results(X, Y, w, folds, flags, dtype=np.float64, stats_only=False, ddof=1):
    """The oracle's outputs for every fold (a list of name -> array or None), computed in ``dtype`` on the
    inputs widened or narrowed to it, with NumPy's warnings off: a NaN is data here."""
    o = OracleCVMatrix(*flags, ddof=ddof, dtype=dtype)
    out = []
    with np.errstate(all="ignore"):
        o.fit(X.astype(dtype), Y.astype(dtype), None if w is None else w.astype(dtype))
        for v in folds:
            if stats_only:
                xtx = xty = None
                st = o.training_statistics(np.asarray(v, dtype=int))
            else:
                (xtx, xty), st = o.training_XTX_XTY(np.asarray(v, dtype=int))
            out.append(dict(zip(NAMES, (xtx, xty) + tuple(st))))
    return out


# ---------------------------------------------------------------------------------------- routes
def _pieces(perm, sizes, sort=False):
    folds, o = [], 0
    for n in sizes:
        f = perm[o:o + n]
        folds.append(np.sort(f) if sort else f)
        o += n
    return folds


def midsize_folds(rng, N, P):
    """tests/test_gpu_parity.py::_midsize_folds: P ragged folds of 33..~3N/P rows plus an empty one."""
    perm = rng.permutation(N)
    cuts = np.sort(rng.choice(np.arange(1, N // 40), P - 1, replace=False)) * 40
    folds = [f for f in np.split(perm, cuts) if len(f) > 32][:P]
    folds.insert(3, np.zeros(0, dtype=int))
    return folds


# name -> (dtype, N, K, M, fold sizes or a builder's name, call style).  The shapes are the smallest at which the
# existing suite establishes that the route is taken (the test named behind each).
ROUTES = {
    "tile_f64": (np.float64, 700, 130, 3, (300, 1, 0, 349, 50), "batched"),        # test_shapes_ragged_empty_and_unaligned
    "tile_f64_odd_k": (np.float64, 700, 129, 3, (300, 1, 0, 349, 50), "batched"),
    "tile_f32_dma": (np.float32, 700, 132, 3, (300, 1, 0, 349, 50), "batched"),    # test_float32_shape_sweep's K
    "sweep_f64": (np.float64, 900, 130, 3, "labels7", "sweep"),                    # test_one_sweep_fit_matches_two_stage
    "fused_f64": (np.float64, 24000, 130, 16, "midsize120", "batched"),            # test_fused_single_split_epilogue_*
    "fused_f32": (np.float32, 24000, 132, 16, "midsize120", "batched"),
    "mid_f64": (np.float64, None, 66, 2, (40, 12, 64, 65), "batched"),             # test_mid_tile_route_shapes
    "mid_f32": (np.float32, None, 260, 20, (64, 9, 150), "batched"),
    "small_f64": (np.float64, 400, 66, 3, (1, 5, 0, 32, 17, 1), "batched"),        # test_small_fold_direct_path
    "loo_rows_f64": (np.float64, 90, 70, 3, (1,) * 24, "batched"),                 # test_leave_one_out_flag_sweep_rows_kernel
    "resident_f32": (np.float32, None, 1024, 3, (16, 1, 0, 7, 16, 2, 9), "resident"),       # test_resident_route_float32
    "resident_f32_36": (np.float32, None, 1024, 2, (32, 17, 1, 25, 0, 32, 20, 9), "resident"),
    "stats_f64": (np.float64, 2500, 130, 16, (900, 33, 0, 567, 1000), "stats"),    # test_training_statistics_streaming_kernel
}
SMALL_BLOCK = {"small_f64": 32, "loo_rows_f64": 32, "resident_f32": 16, "resident_f32_36": 32}
_EXTRA_ROWS = {"mid_f64": 57, "mid_f32": 57, "resident_f32": 40, "resident_f32_36": 40}


def route_geometry(route):
    """(dtype, N, K, M, folds, style, rows): the folds of the route's shape and the rows a loader can get wrong
    (name -> row index): the first row of a fold (the last one), the last row of a fold whose size is no multiple of 16
    (the earliest such), a row
    in no fold where the shape leaves one, and on the small routes the last row of a fold smaller than the
    operand block."""
    dtype, N, K, M, spec, style = ROUTES[route]
    rng = np.random.default_rng(sorted(ROUTES).index(route) + 4100)
    if spec == "labels7":
        labels = rng.integers(0, 7, size=N)
        folds = [np.flatnonzero(labels == k) for k in dict.fromkeys(labels.tolist())]
    elif spec == "midsize120":
        folds = midsize_folds(rng, N, 120)
    else:
        if N is None:
            N = sum(spec) + _EXTRA_ROWS[route]
        folds = _pieces(rng.permutation(N), spec, sort=route.startswith(("mid", "resident")))
    # (the first row of the last fold and the last row of an early one: a load that runs past one fold's rows, or
    # starts before them, lands on a row that is poisoned in another fold)
    first = next(f for f in folds[::-1] if len(f))
    partial = next(f for f in folds if len(f) % 16 and len(f) > 1) if max(map(len, folds)) > 1 else folds[0]
    rows = {"first": int(first[0]), "last_partial": int(partial[-1])}
    used = np.zeros(N, bool)
    for f in folds:
        used[f] = True
    if not used.all():
        rows["no_fold"] = int(np.flatnonzero(~used)[-1])
    if route in SMALL_BLOCK:
        short = next(f for f in folds[::-1] if 1 < len(f) < SMALL_BLOCK[route]) if max(map(len, folds)) > 1 else folds[7]
        rows["last_short"] = int(short[-1])
    return dtype, N, K, M, folds, style, rows


def route_columns(K):
    """Column 0, the last column, the two columns on either side of the first tile edge."""
    return list(dict.fromkeys(c for c in (0, K - 1, 63, 64) if 0 <= c < K))


_CLEAN = {}


def route_problem(route):
    """The clean problem of a route (built once, never written to): X = N(0, 1) + 0.5 like the suite's, Y
    uniform, weights uniform with zeros at rows that are none of the route's poison rows."""
    if route not in _CLEAN:
        dtype, N, K, M, folds, style, rows = route_geometry(route)
        rng = np.random.default_rng(sorted(ROUTES).index(route) + 5100)
        X = (rng.standard_normal((N, K)) + 0.5).astype(dtype)
        Y = rng.random((N, M)).astype(dtype)
        w = (rng.random(N) + 0.01).astype(dtype)
        keep = set(rows.values()) | {pair_row(r, N) for r in rows.values()}
        zero = [int(r) for r in rng.choice(N, max(N // 14, 4), replace=False) if int(r) not in keep]
        w[zero] = 0
        for a in (X, Y, w):
            a.setflags(write=False)
        _CLEAN[route] = (X, Y, w)
    return _CLEAN[route]


def containment_cases(route):
    """(kind, flags, row name, col) of a route: the five NaN / Inf kinds with the flags all on and all off, a NaN
    weight once, and on float64 the overflowing cell -- with the flags off only at a row in no fold (inside a fold
    row and column c of G - G_val are differences of two numbers near 1e200: rounding noise in the oracle as in
    the product).  Columns and rows cycle so that each position appears at least once per route.

    Two things the shapes themselves decide.  The folds of the tile, fused, sweep and statistics shapes, taken from
    the tests that establish those routes, cover every row: there is no row in no fold there (for the sweep there
    cannot be one), so that position, and with it the overflowing cell with the flags off, runs on the mid-tile,
    small-fold, leave-one-out and resident shapes only.  ``training_statistics`` returns nothing but None with every
    flag off: the statistics route runs scaling only, (False, False, True, True), in place of all off."""
    dtype, N, K, M, folds, style, rows = route_geometry(route)
    cols, rnames = route_columns(K), list(rows)
    second = (False, False, True, True) if style == "stats" else OFF        # (no flag: no statistics to look at)
    todo = [(k, fl) for fl in (ON, second) for k in X_KINDS + ("nan_y",)] + [("nan_w", ON)]
    if dtype is np.float64:
        todo.append(("overflow_x", ON))
        if "no_fold" in rows and style != "stats":
            todo.append(("overflow_x", OFF))
    out = []
    for i, (kind, fl) in enumerate(todo):
        rn = rnames[(i + i // len(cols)) % len(rnames)]
        if kind == "overflow_x" and not any(fl):
            rn = "no_fold"
        out.append((kind, fl, rn, cols[i % len(cols)]))
    return out


def random_defect(rng, X, Y, w, flags):
    """One defect for a randomised case (tools/fuzz_all.py, fuzz_small.py under CVM_FUZZ_HARD=1): a kind that the
    case's inputs allow -- the overflowing cell only in float64 with scale_X on, where it poisons its whole row and
    column instead of leaving differences of numbers near 1e200 -- at a random row and at a column on a tile edge or
    anywhere.  Returns (X, Y, w, (kind, row, col))."""
    N, K = X.shape
    kinds = list(X_KINDS[:3]) + (["nan_y"] if Y is not None else []) + (["nan_x_zero_w", "nan_w"] if w is not None else [])
    if X.dtype == np.float64 and flags[2]:
        kinds.append("overflow_x")
    kind = str(rng.choice(kinds))
    row = int(rng.integers(0, N))
    col = int(rng.choice(route_columns(K) + [int(rng.integers(0, K))]))
    if kind == "overflow_x" and w is not None and w[row] == 0:
        kind = "nan_x"
    return poisoned(X, Y, w, kind, row, col) + ((kind, row, col),)


def symmetric_where_finite(x):
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return bool(np.array_equal(fin, fin.T) and np.array_equal(x[fin], x.T[fin]))


def case_id(case):
    kind, fl, rn, col = case
    return f"{kind}-{''.join('1' if f else '0' for f in fl)}-{rn}-c{col}"


# ---------------------------------------------------------------------------------------- cancellation
LADDER = {np.float64: (1.0, 1e2, 1e4, 1e6), np.float32: (1.0, 3.0, 10.0, 30.0)}
LADDER_MIN_ERR = {np.float64: 1e-10, np.float32: 1e-5}        # from the second rung on: the rung tests cancellation
LADDER_MAX_YARD = 0.1          # a yardstick above it is no longer a result: twice it bounds nothing, the comparison is not made
# (route, offset, output) with such a yardstick in some run and fold -- all of them, test_hard_inputs_oracle.py holds
# the list to that: XTY on the top float64 rung of the two shapes with the most rows (X and Y are independent, the
# centred XTY has no large entry to carry the norm); their XTX and statistics are compared there as on every rung
LADDER_BEYOND = {("fused_f64", 1e6, "XTY"), ("tile_f64", 1e6, "XTY")}
LADDER_RUNS = (("weighted", ON, True), ("unweighted", ON, False), ("centre_only", CENTRE_ONLY, True))
# route -> (route of ROUTES whose shape it takes, fold sizes or None for the route's own, folds checked)
LADDER_ROUTES = {
    "tile_f64": ("tile_f64", (300, 50), (0, 1)),
    "fused_f64": ("fused_f64", None, (0, 5)),
    "mid_f64": ("mid_f64", None, (0, 1, 2, 3)),
    "small_f64": ("small_f64", None, (0, 3, 4)),
    "tile_f32_dma": ("tile_f32_dma", (300, 50), (0, 1)),
    "resident_f32": ("resident_f32", None, (0, 3, 6)),
}


def offset_problem(N, K, M, off, dtype, seed):
    """X = N(0, 1) + off (1 + U(0, 1)) per column, Y likewise, weights U(0.05, 1.05): mean / std is about
    1.5 off, and subtract-and-correct loses about eps (mean / std)^2."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, K)) + off * (1.0 + rng.random((1, K)))
    Y = rng.standard_normal((N, M)) + off * (1.0 + rng.random((1, M)))
    w = rng.random(N) + 0.05
    return X.astype(dtype), Y.astype(dtype), w.astype(dtype)


def ladder_problem(route, off):
    """(X, Y, w, folds, checked) of a ladder route at one rung."""
    base, sizes, checked = LADDER_ROUTES[route]
    dtype, N, K, M, folds, style, rows = route_geometry(base)
    if sizes is not None:
        folds = _pieces(np.random.default_rng(77).permutation(N), sizes)
    X, Y, w = offset_problem(N, K, M, off, dtype, seed=int(1000 + 10 * np.log10(off) + sorted(ROUTES).index(base)))
    return X, Y, w, folds, checked


def exact_dtype():
    return np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64


def exact_training_matrices(X, Y, w, val, flags, ddof=1, cols=None):
    """The training-set matrices and statistics by their definition (``naive_training_matrices``: centre and
    scale the training rows, then multiply) in extended precision where ``long double`` has one, else in
    float64 (within 3e-15 of the extended result on every rung).  ``cols``: for these columns of X only (centring
    and scaling are per column: the block XTX[cols, cols] and the rows XTY[cols] of the whole problem's).
    Returns name -> array or None."""
    N = X.shape[0]
    keep = np.ones(N, bool)
    keep[np.asarray(val, dtype=int)] = False
    Xc = X if cols is None else X[:, cols]
    with np.errstate(all="ignore"):
        (xtx, xty), st = naive_training_matrices(Xc, Y, w, np.flatnonzero(keep), *flags, ddof, dtype=exact_dtype())
    return dict(zip(NAMES, (xtx, xty) + tuple(st)))


def cut_columns(res, cols):
    """The entries of one fold's outputs (name -> array or None) that belong to the columns ``cols`` of X."""
    if cols is None:
        return res
    out = dict(res)
    if out.get("XTX") is not None:
        out["XTX"] = np.asarray(out["XTX"])[np.ix_(cols, cols)]
    for n in ("XTY", ):
        if out.get(n) is not None:
            out[n] = np.asarray(out[n])[cols, :]
    for n in ("muX", "sdX"):
        if out.get(n) is not None:
            out[n] = np.asarray(out[n]).reshape(1, -1)[:, cols]
    return out


def ladder_columns(route):
    """The extended-precision product costs N K^2 slow multiplications: where that is beyond about 2e7 the ladder
    looks at a fixed sample of the columns -- the tile edges and seeded random ones, as many as that budget
    allows -- and measures error and yardstick on the same entries."""
    dtype, N, K, M, folds, style, rows = route_geometry(LADDER_ROUTES[route][0])
    return sample_columns(N, K)


def sample_columns(N, K):
    """The column sample of ``ladder_columns`` for a problem of N rows and K columns (None: all columns)."""
    n = int(np.sqrt(2e7 / N))
    if n >= K:
        return None
    edges = [c for c in (0, 1, 62, 63, 64, 65, 127, 128, K - 2, K - 1) if c < K]
    rest = np.setdiff1d(np.arange(K), edges)
    pick = np.random.default_rng(K).choice(rest, max(n - len(edges), 0), replace=False)
    return np.sort(np.concatenate([edges, pick]).astype(int))


def nerr(got, exact):
    """Norm-wise max error, in the arithmetic of ``exact``."""
    exact = np.asarray(exact)
    d = np.abs(np.asarray(got).astype(exact.dtype).reshape(exact.shape) - exact).max()
    return float(d / max(np.abs(exact).max(), TINY))


def row_orders(N):
    """The three fixed row orders of the ladder's yardstick: as given, reversed, a seeded shuffle."""
    return (np.arange(N), np.arange(N)[::-1], np.random.default_rng(2024).permutation(N))


_LADDER_REF = {}


def ladder_reference(route, off, run):
    """Per checked fold: (exact outputs, the oracle's error against them in the route's element type on the rows as
    given, the yardstick), computed once per rung and run and shared by every test that needs it.  The yardstick is
    the largest oracle error over the three row orders of ``row_orders``: the error of a cancelling sum is one draw
    per summation order, and on an output of three entries (sdY at M = 3) a single draw can be ten times below the
    next (tile shape, offset 1e4, weighted, fold 1: 2.7e-8 as given, 3.2e-7 reversed, 2.6e-7 shuffled)."""
    key = (route, off, run)
    if key not in _LADDER_REF:
        flags, weighted = next((fl, wt) for n, fl, wt in LADDER_RUNS if n == run)
        X, Y, w, folds, checked = ladder_problem(route, off)
        wt = w if weighted else None
        cols = ladder_columns(route)
        N = X.shape[0]
        per_order = []
        for p in row_orders(N):
            inv = np.empty(N, dtype=int)
            inv[p] = np.arange(N)
            per_order.append(oracle_fold_results(X[p], Y[p], None if wt is None else wt[p], [inv[folds[f]] for f in checked],
                                                 flags, dtype=X.dtype.type))
        out = {}
        for i, f in enumerate(checked):
            ex = exact_training_matrices(X, Y, wt, folds[f], flags, cols=cols)
            errs = [{n: nerr(cut_columns(o[i], cols)[n], ex[n]) for n in NAMES if ex[n] is not None} for o in per_order]
            out[f] = (ex, errs[0], {n: max(e[n] for e in errs) for n in errs[0]})
        _LADDER_REF[key] = out
    return _LADDER_REF[key]


def ladder_floor(dtype):
    return TOL64 if dtype is np.float64 else fp32_floor()


def report(line):
    """CVM_HARD_REPORT=path: one line per ladder comparison (calibration runs)."""
    path = os.environ.get("CVM_HARD_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---------------------------------------------------------------------------------------- scale spread
# (dtype, span, wspan); run on the tile, mid-tile and small-fold shapes
SPREADS = ((np.float64, 8, 6), (np.float64, 100, 6), (np.float32, 4, 3))
# (the small-fold shape has one entry in ROUTES, float64: its float32 run takes the element type from SPREADS)
SPREAD_ROUTES = {np.float64: ("tile_f64", "mid_f64", "small_f64"), np.float32: ("tile_f32_dma", "mid_f32", "small_f64")}
SPREAD_MAX_ERR = {np.float64: 1e-12, np.float32: 1e-5}


def spread_problem(N, K, M, span, wspan, dtype, seed):
    """Columns of X and Y scaled by 10^U(-span, span), weights 10^U(-wspan, wspan).  A standard deviation at or
    below ten times the resolution of the element type counts as zero (1e-14 in float64, 1e-17 in extended
    precision): exponents drawn between -19.5 and -12.5, where the float64 definition and the exact one differ
    by design, are moved down by 8, to columns that are constant for both.  Returns the column exponents of X as
    well (the decade groups of ``decade_groups``)."""
    rng = np.random.default_rng(seed)
    ex = rng.uniform(-span, span, K)
    ey = rng.uniform(-span, span, M)
    ex = np.where((ex > -19.5) & (ex < -12.5), ex - 8.0, ex)
    ey = np.where((ey > -19.5) & (ey < -12.5), ey - 8.0, ey)
    X = (rng.standard_normal((N, K)) + 0.5) * 10.0 ** ex
    Y = (rng.standard_normal((N, M)) + 0.5) * 10.0 ** ey
    w = 10.0 ** rng.uniform(-wspan, wspan, N)
    return X.astype(dtype), Y.astype(dtype), w.astype(dtype), ex


def spread_case(route, span, wspan, dtype):
    """The spread problem on a route's shape and folds, in ``dtype``."""
    _, N, K, M, folds, style, rows = route_geometry(route)
    X, Y, w, ex = spread_problem(N, K, M, span, wspan, dtype, seed=300 + span + sorted(ROUTES).index(route))
    return X, Y, w, folds, ex


def decade_groups(ex):
    """Columns grouped by decade of their scale: a list of index arrays."""
    dec = np.floor(ex).astype(int)
    return [np.flatnonzero(dec == d) for d in np.unique(dec)]


def blockwise_errors(got, ref, groups):
    """Per (group, group) block of XTX: max |got - ref| over the block against the block's natural scale, the root
    of the product of the two groups' largest diagonal entries of ``ref`` -- for a diagonal block that is the
    block's own max (the matrix is positive semi-definite); an off-diagonal block of a few entries has no scale of
    its own (a centred cross product may be anywhere near zero), and Cauchy-Schwarz bounds it by this one."""
    ref = np.asarray(ref)
    got = np.asarray(got).astype(ref.dtype)
    top = [np.abs(np.diagonal(ref)[g]).max() for g in groups]
    return np.array([[float(np.abs(got[np.ix_(ga, gb)] - ref[np.ix_(ga, gb)]).max() / max(np.sqrt(top[a]) * np.sqrt(top[b]), TINY))
                      for b, gb in enumerate(groups)] for a, ga in enumerate(groups)])


def assert_blockwise(got, ref, groups, tol=TOL64, what=""):
    """Every (decade, decade) block of XTX within ``tol`` of its scale: the small columns are seen."""
    e = blockwise_errors(got, ref, groups)
    a, b = np.unravel_index(np.argmax(e), e.shape)
    assert e[a, b] <= tol, f"{what}: decades {a} x {b}: {e[a, b]:.3e} > {tol}"
