"""Cases, references and assertion functions of the hard-input tests of streaming cross-validation and of the unions of
folds (tests/test_gpu_stream_hard.py on the GPU; tests/test_stream_hard_oracle.py checks on the CPU that every case
meets its own conditions for the oracle alone, and that the assertion functions below catch a seeded defect in a
NumPy model of the sums).  NumPy and the oracle only: nothing here touches the product.  The builders, gates and
constants are those of tests/hard_input_cases.py (hc), the fold layout is tests/unions_cases.py's (uc), the chunkings
B and C are tests/streaming_cases.py's (sc).

Design: uc.N = 203 rows in five folds of uc.SIZES = (67, 33, 41, 40, 22) rows dealt by a seeded label permutation,
K = 130 and M = 3 (an off-diagonal tile, an odd K; hc.route_columns gives columns 0, 63, 64, 129), for containment
K = 7 and M = 1 as well (under CVM_PAD=0: rows that are not 16-byte aligned, the fallback Gram kernel).

Chunkings: B (rows 0:80, an empty chunk, the single row 80, the rest), C (one fold per chunk), S (13 chunks of 16
rows, the last of 11: many accumulations), W (rows by ascending weight in 8 chunks: the order in which a running sum
in the element type loses the small terms).

Items: the five folds and seven unions of them whose complements hold 136, 181, 103, 148, 67, 40 and 22 rows.  An
item is ("fold", f) or ("union", (f, g, ...)); results travel as item -> {name -> array or None} with hc.NAMES."""

import functools

import numpy as np

import hard_input_cases as hc
import streaming_cases as sc
import unions_cases as uc

K, M = 130, 3
SMALL = (7, 1)
N, P = uc.N, uc.P
UNIONS = ((0,), (4,), (0, 1), (1, 4), (1, 2, 3, 4), (0, 1, 2, 4), (0, 1, 2, 3))
COMPLEMENT_ROWS = (136, 181, 103, 148, 67, 40, 22)
FOLD_ITEMS = tuple(("fold", f) for f in range(P))
UNION_ITEMS = tuple(("union", S) for S in UNIONS)
ITEMS = FOLD_ITEMS + UNION_ITEMS
SMALLEST = ("union", (0, 1, 2, 3))              # leaves the 22 rows of fold 4
DTYPES = (np.float64, np.float32)
MUTANTS = ("stale_slot", "float32_accumulator", "nan_dropped", "union_stats_of_wrong_fold", "union_unordered")


def item_id(item):
    return item[0] + ("+".join(str(f) for f in item[1]) if item[0] == "union" else str(item[1]))


@functools.lru_cache(maxsize=None)
def design():
    """(labels, folds): folds[f] = ascending rows of fold f (fold position = label)."""
    labels = np.random.default_rng(5).permutation(np.repeat(np.arange(P), uc.SIZES)).astype(np.int64)
    folds = tuple(np.flatnonzero(labels == f) for f in range(P))
    for a in (labels,) + folds:
        a.setflags(write=False)
    return labels, folds


def validation_rows(item, folds=None):
    folds = design()[1] if folds is None else folds
    return folds[item[1]] if item[0] == "fold" else uc.union_indices(folds, item[1])


def chunk_rows(name, labels, w=None):
    """The row-index arrays of a chunking in feeding order: sc's B and C, and S and W (``w``: the weights)."""
    n = len(labels)
    if name in ("B", "C"):
        return sc.chunk_rows(name, labels)
    if name == "S":
        return [np.arange(a, min(a + 16, n)) for a in range(0, n, 16)]
    if name == "W":
        return [np.asarray(r) for r in np.array_split(np.argsort(w, kind="stable"), 8)]
    raise KeyError(name)


def oracle_items(X, Y, w, flags, dtype=np.float64, items=ITEMS, folds=None):
    """The oracle's outputs per item: a fold's rows, or the concatenated rows of a union, as validation indices."""
    res = hc.oracle_fold_results(X, Y, w, [validation_rows(i, folds) for i in items], flags, dtype=dtype)
    return dict(zip(items, res))


# ---------------------------------------------------------------------------------------- containment
# where the poisoned cell sits: name -> (row, the chunking under which the row is what the name says)
def poison_rows():
    labels, folds = design()
    lone = int(folds[3][len(folds[3]) // 2])
    first = int(np.flatnonzero(labels[:16] == labels[0])[0])                  # = 0
    same = int(192 + np.flatnonzero(labels[192:] == labels[first])[0])        # a row of S's last chunk in the same fold
    other = int(192 + np.flatnonzero(labels[192:] != labels[first])[0])
    return {"one_row": (80, "B"),                  # the single row of B's one-row chunk
            "chunk_first": (48, "S"),              # the first row of a chunk
            "last_partial": (N - 1, "S"),          # the last row of a chunk of 11 rows
            "lone_fold": (lone, "C"),              # a row of a fold that has rows in exactly one chunk
            "pair_same_fold": ((first, same), "B"),        # +Inf in the first chunk, -Inf in the last, one fold
            "pair_two_folds": ((first, other), "S")}       # ... in two folds


ROW_NAMES = ("one_row", "chunk_first", "last_partial", "lone_fold")


def containment_cases(k, dtype):
    """(kind, flags, row name, col): every kind of hc.KINDS with the flags all on and all off, cycling through the row
    positions and hc.route_columns(k); ``nan_x_zero_w`` in the one-row chunk; the two +Inf / -Inf pairs across chunks.
    As in hc.containment_cases a NaN weight runs once, and the overflowing cell (float64) with the flags on only:
    every row is in a fold here, and with the flags off row and column c of G - U_f are differences of numbers near
    1e200, rounding noise in the oracle as in the product."""
    cols = hc.route_columns(k)
    todo = [(kd, fl) for fl in (hc.ON, hc.OFF) for kd in hc.X_KINDS + ("nan_y",)] + [("nan_w", hc.ON)]
    if dtype is np.float64:
        todo.append(("overflow_x", hc.ON))
    out = []
    for i, (kind, fl) in enumerate(todo):
        rn = "one_row" if kind == "nan_x_zero_w" else ROW_NAMES[(i + i // len(cols)) % len(ROW_NAMES)]
        out.append((kind, fl, rn, cols[i % len(cols)]))
    for i, fl in enumerate((hc.ON, hc.OFF)):
        out += [("infpair_x", fl, "pair_same_fold", cols[i % len(cols)]), ("infpair_x", fl, "pair_two_folds", cols[-1 - i % len(cols)])]
    return out


def case_id(case):
    kind, fl, rn, col = case
    return f"{kind}-{''.join('1' if f else '0' for f in fl)}-{rn}-c{col}"


def case_chunking(case):
    return poison_rows()[case[2]][1]


def case_fold(case):
    """The fold of the poisoned row (of the +Inf row of a pair)."""
    row = poison_rows()[case[2]][0]
    return int(design()[0][row if np.isscalar(row) else row[0]])


def case_items(case):
    """The items of a case: the poisoned fold is inside some unions of UNIONS and outside others; it is added as a
    union of its own where UNIONS has none."""
    own = ("union", (case_fold(case),))
    return ITEMS if own in ITEMS else ITEMS + (own,)


@functools.lru_cache(maxsize=None)
def clean_problem(k, m, dtype_name):
    """X = N(0, 1) + 0.5 like the suite's, Y uniform, weights U(0.05, 1.05) with a tenth zero at rows that are none of
    the poison rows.  Built once, never written to."""
    rng = np.random.default_rng(7100 + k)
    dt = np.dtype(dtype_name).type
    X = (rng.standard_normal((N, k)) + 0.5).astype(dt)
    Y = rng.random((N, m)).astype(dt)
    w = (rng.random(N) + 0.05).astype(dt)
    keep = set()
    for r, _ in poison_rows().values():
        for q in np.atleast_1d(r):
            keep |= {int(q), hc.pair_row(int(q), N)}
    zero = [int(r) for r in rng.choice(N, N // 10 + len(keep), replace=False) if int(r) not in keep][:N // 10]
    w[zero] = 0
    for a in (X, Y, w):
        a.setflags(write=False)
    return X, Y, w


def poisoned_problem(k, m, dtype_name, case):
    kind, fl, rn, col = case
    X, Y, w = clean_problem(k, m, dtype_name)
    row = poison_rows()[rn][0]
    if rn.startswith("pair_"):
        X = X.copy()
        X[row[0], col], X[row[1], col] = np.inf, -np.inf
        return X, Y, w
    return hc.poisoned(X, Y, w, kind, row, col)


@functools.lru_cache(maxsize=None)
def containment_reference(k, m, dtype_name, case):
    """(X, Y, w, the float64 oracle per item, the oracle's float32 run per item or None, the float64 oracle's
    ``training_statistics`` per fold, its float32 run or None) of one case.  The statistics call has its own flag map
    and returns nothing with the flags off: it is compared with the flags on only."""
    dt = np.dtype(dtype_name).type
    flags = case[1]
    X, Y, w = poisoned_problem(k, m, dtype_name, case)
    items = case_items(case)
    folds = design()[1]
    ref = oracle_items(X, Y, w, flags, items=items)
    ref32 = oracle_items(X, Y, w, flags, np.float32, items) if dt is np.float32 else None
    st = st32 = None
    if flags == hc.ON:
        st = hc.oracle_fold_results(X, Y, w, folds, flags, stats_only=True)
        st32 = hc.oracle_fold_results(X, Y, w, folds, flags, dtype=np.float32, stats_only=True) if dt is np.float32 else None
    return X, Y, w, ref, ref32, st, st32


def assert_containment(got, reference, case, dtype, what=""):
    """hc.compare_fold's rule (mask equal to the oracle's element for element, the suite's gates on the finite entries,
    XTX symmetric with a symmetric mask, no vacuous comparison) for every item of ``got`` (item -> outputs)."""
    X, Y, w, ref, ref32, st, st32 = reference
    kind, fl, rn, col = case
    assert got, what
    for item, g in got.items():
        hc.compare_fold(g, ref[item], None if ref32 is None else ref32[item], kind, col, dtype, f"{what} {case_id(case)} {item_id(item)}")


def assert_containment_statistics(got, reference, case, dtype, what=""):
    """The same for ``training_statistics_batched`` (``got``: one dict per fold with XTX and XTY None)."""
    X, Y, w, ref, ref32, st, st32 = reference
    kind, fl, rn, col = case
    for f in range(P):
        hc.compare_fold(got[f], st[f], None if st32 is None else st32[f], kind, col, dtype, f"{what} {case_id(case)} statistics fold{f}")


# ---------------------------------------------------------------------------------------- cancellation ladder
# (dtype name, offset, item id, output) whose yardstick is above hc.LADDER_MAX_YARD in some run: not compared.  Held by
# tests/test_stream_hard_oracle.py to exactly what the oracle alone yields, and to the condition that it names only
# XTX and XTY, only on the top rung, only of unions whose complement is the 22-row fold.
LADDER_BEYOND = {("float64", 1e6, "union0+1+2+3", "XTX"), ("float64", 1e6, "union0+1+2+3", "XTY"),
                 ("float32", 30.0, "union0+1+2+3", "XTX")}
LADDER_CHUNKINGS = ("B", "C", "S")
DRIFT = "drift"                 # the extra run: weighted, all flags on, the column means drift from chunk to chunk of S
SPLIT_RUNG = {np.float64: 1e4, np.float32: 10.0}
SPLIT_ITEMS = (("fold", 0), ("fold", 4), SMALLEST)


def ladder_runs():
    return tuple(n for n, _, _ in hc.LADDER_RUNS) + (DRIFT,)


def run_settings(run):
    """(flags, weighted) of a run."""
    if run == DRIFT:
        return hc.ON, True
    return next((fl, wt) for n, fl, wt in hc.LADDER_RUNS if n == run)


@functools.lru_cache(maxsize=None)
def ladder_problem(dtype_name, off, run):
    """(X, Y, w or None) of a rung: hc.offset_problem on the design's shape.  The drift run adds off * c / 13 to the
    rows of chunk c of chunking S: the sums are the same sums, fed chunks whose column means differ."""
    dt = np.dtype(dtype_name).type
    X, Y, w = hc.offset_problem(N, K, M, off, dt, seed=int(round(7 + 10 * np.log10(off))))
    if run == DRIFT:
        shift = np.zeros((N, 1))
        for c, r in enumerate(chunk_rows("S", design()[0])):
            shift[r] = off * c / 13
        X = (X.astype(np.float64) + shift).astype(dt)
    flags, weighted = run_settings(run)
    for a in (X, Y, w):
        a.setflags(write=False)
    return X, Y, (w if weighted else None)


def _reference(X, Y, w, folds, items, flags, cols=None):
    """item -> (exact outputs, the oracle's error in the element type of X on the rows as given, the yardstick: its
    largest error over hc.row_orders)."""
    n = X.shape[0]
    per_order = []
    for p in hc.row_orders(n):
        inv = np.empty(n, dtype=int)
        inv[p] = np.arange(n)
        per_order.append(hc.oracle_fold_results(X[p], Y[p], None if w is None else w[p], [inv[validation_rows(i, folds)] for i in items],
                                                flags, dtype=X.dtype.type))
    out = {}
    for j, item in enumerate(items):
        ex = hc.exact_training_matrices(X, Y, w, validation_rows(item, folds), flags, cols=cols)
        errs = [{nm: hc.nerr(hc.cut_columns(o[j], cols)[nm], ex[nm]) for nm in hc.NAMES if ex[nm] is not None} for o in per_order]
        out[item] = (ex, errs[0], {nm: max(e[nm] for e in errs) for nm in errs[0]})
    return out


@functools.lru_cache(maxsize=None)
def ladder_reference(dtype_name, off, run):
    X, Y, w = ladder_problem(dtype_name, off, run)
    return _reference(X, Y, w, design()[1], ITEMS, run_settings(run)[0])


@functools.lru_cache(maxsize=None)
def split_problem(dtype_name):
    """One rung on uc.split_design's shape (1200 rows, five folds of 240, two chunks of 600), weighted, all flags on:
    (X, Y, w, labels, folds, cols, item -> reference)."""
    dt = np.dtype(dtype_name).type
    _, _, _, labels, folds = uc.split_design(dtype_name)
    off = SPLIT_RUNG[dt]
    X, Y, w = hc.offset_problem(1200, K, M, off, dt, seed=int(round(7 + 10 * np.log10(off))))
    cols = hc.sample_columns(1200, K)          # (hc.ladder_columns's rule: a budget of 2e7 extended-precision multiplications)
    return X, Y, w, labels, folds, cols, _reference(X, Y, w, folds, SPLIT_ITEMS, hc.ON, cols)


def assert_ladder(got, reference, dtype, off, run, route, cols=None, beyond=None):
    """The gate of the ladder for every item of ``got``: every output finite, and
    err(got vs exact) <= 2 x yardstick + hc.ladder_floor(dtype) wherever the yardstick is a result (at most
    hc.LADDER_MAX_YARD; beyond it the comparison must be on LADDER_BEYOND and is not made).  One hc.report line per
    comparison."""
    beyond = LADDER_BEYOND if beyond is None else beyond
    floor = hc.ladder_floor(dtype)
    name = np.dtype(dtype).name
    bad = []
    assert got, route
    for item, res in got.items():
        exact, as_given, yard = reference[item]
        g = hc.cut_columns(res, cols)
        for nm, y in yard.items():
            assert g[nm] is not None and np.isfinite(np.asarray(g[nm], dtype=np.float64)).all(), (route, name, off, run, item_id(item), nm)
            if y > hc.LADDER_MAX_YARD:
                assert (name, off, item_id(item), nm) in beyond, (name, off, item_id(item), nm, y)
                continue
            err = hc.nerr(g[nm], exact[nm])
            hc.report(f"{route}\t{name}\t{off:g}\t{run}\t{item_id(item)}\t{nm}\t{err:.3e}\t{as_given[nm]:.3e}\t{y:.3e}\t{err / max(y, 1e-300):.2f}")
            if not err <= 2 * y + floor:
                bad.append((item_id(item), nm, err, y))
    assert not bad, f"{route} {name} offset {off:g} {run}: error above 2 x the oracle's own + {floor:.1e}; (item, output, err, yardstick): {bad}"


# ---------------------------------------------------------------------------------------- scale spread
SPREAD_CHUNKINGS = ("B", "W")
# The seed of each spread problem: 300 + span + j with the first j at which the oracle alone, in the element type, is
# within hc.SPREAD_MAX_ERR of the exact result for all twelve items (tests/test_stream_hard_oracle.py asserts that it
# is).  Under weights spread over 2 wspan decades the rows a large union removes hold up to 99 % of the total weight,
# and the oracle's own G - sum U_f then cancels: in float64 2.5e-12 at j = 0 of span 8 (1.1e-13 at j = 1); in float32
# between 1.2e-5 and 5e-4 for the union that leaves 22 rows at every j below 149, 9.9e-6 there.  The float32 problem
# is therefore a favourable draw for the oracle -- which makes the float32 gate, twice the oracle's own float32 error,
# the narrower for it.  The cancellation itself is the ladder's subject.
SPREAD_SEED_STEP = {("float64", 8): 1, ("float64", 100): 0, ("float32", 4): 149}


@functools.lru_cache(maxsize=None)
def spread_reference(dtype_name, span, wspan):
    """(X, Y, w, decade groups, flags -> (float64 oracle per item, the oracle's float32 run or None), item -> scales of
    the float32 means or {}) for the flags all on and centring only."""
    dt = np.dtype(dtype_name).type
    X, Y, w, ex = hc.spread_problem(N, K, M, span, wspan, dt, seed=300 + span + SPREAD_SEED_STEP[(dtype_name, span)])
    for a in (X, Y, w):
        a.setflags(write=False)
    refs = {}
    for flags in (hc.ON, hc.CENTRE_ONLY):
        refs[flags] = (oracle_items(X, Y, w, flags), oracle_items(X, Y, w, flags, np.float32) if dt is np.float32 else None)
    scales = {i: (hc.mean_scales(X, Y, w, validation_rows(i)) if dt is np.float32 else {}) for i in ITEMS}
    return X, Y, w, hc.decade_groups(ex), refs, scales


def assert_spread(got, reference, flags, dtype, what=""):
    """All flags on: the gates tests/test_gpu_hard_inputs.py uses for its spread cases (matrices norm-wise, statistics
    element-wise, the float32 means against hc.mean_scales).  Centring only: every (decade, decade) block of XTX
    against its own scale -- hc.assert_blockwise with hc.TOL64 in float64; in float32 hc.gate_float32's rule per
    block, the yardstick being the block error of the oracle's own float32 run."""
    X, Y, w, groups, refs, scales = reference
    ref, ref32 = refs[flags]
    assert got, what
    for item, g in got.items():
        w_ = f"{what} {item_id(item)}"
        if flags == hc.ON:
            for nm in hc.NAMES:
                if nm in hc.STAT_NAMES:
                    gate = hc.gate_stats(hc.STAT_RTOL[dtype], scale=scales[item].get(nm))
                else:
                    gate = hc.gate_float64() if dtype is np.float64 else hc.gate_float32(ref32[item][nm])
                hc.assert_matches_oracle_where_finite(np.reshape(g[nm], np.shape(ref[item][nm])), ref[item][nm], gate, f"{w_} {nm}")
        elif dtype is np.float64:
            hc.assert_blockwise(g["XTX"], ref[item]["XTX"], groups, what=f"{w_} XTX")
        else:
            assert np.isfinite(np.asarray(g["XTX"], dtype=np.float64)).all(), w_
            err = hc.blockwise_errors(g["XTX"], ref[item]["XTX"], groups)
            yard = hc.blockwise_errors(ref32[item]["XTX"], ref[item]["XTX"], groups)
            over = np.argwhere(~(err <= 2 * yard + hc.ladder_floor(dtype)))
            assert over.size == 0, (f"{w_} XTX: decades {over[0].tolist()}: {err[tuple(over[0])]:.3e} > 2 x "
                                    f"{yard[tuple(over[0])]:.3e} + {hc.ladder_floor(dtype)}")


# ---------------------------------------------------------------------------------------- the NumPy model and its defects
def model_accumulate(X, Y, w, labels, rows, dt, mutant=None):
    """tests/test_streaming_host.py's accumulate (per chunk and fold the raw update formed in ``dt``, added to a
    float64 accumulator, rounded to ``dt`` once), with one seeded defect:
      stale_slot            a fold that is absent from a chunk gets the update the slot last held
      float32_accumulator   the accumulator is float32
      nan_dropped           the accumulate adds only where the partial compares greater or less than zero"""
    k, m = X.shape[1], Y.shape[1]
    at = np.float32 if mutant == "float32_accumulator" else np.float64
    keys = ("U", "V", "s", "q", "sy", "qy", "sw", "nz")
    acc = [dict(U=np.zeros((k, k), at), V=np.zeros((k, m), at), s=np.zeros(k, at), q=np.zeros(k, at), sy=np.zeros(m, at),
                qy=np.zeros(m, at), sw=at(0), nz=at(0)) for _ in range(P)]
    slot = [None] * P

    def add(a, upd):
        for key in keys:
            u = np.asarray(upd[key], dtype=np.float64)
            if mutant == "nan_dropped":
                u = np.where((u > 0) | (u < 0), u, 0.0)
            a[key] = (a[key] + u.astype(at)).astype(at)
    with np.errstate(all="ignore"):
        for r in rows:
            if len(r) == 0:
                continue
            for f in range(P):
                rf = r[labels[r] == f]
                if rf.size == 0:
                    if mutant == "stale_slot" and slot[f] is not None:
                        add(acc[f], slot[f])
                    continue
                Xc, Yc = X[rf].astype(dt), Y[rf].astype(dt)
                wc = None if w is None else w[rf].astype(dt).reshape(-1, 1)
                WX = Xc if wc is None else Xc * wc
                WX64, X64, Y64 = WX.astype(np.float64), Xc.astype(np.float64), Yc.astype(np.float64)
                WY64 = Y64 if wc is None else Y64 * wc.astype(np.float64)
                slot[f] = dict(U=WX.T @ Xc, V=WX.T @ Yc, s=WX64.sum(0), q=(WX64 * X64).sum(0), sy=WY64.sum(0), qy=(WY64 * Y64).sum(0),
                               sw=float(rf.size) if wc is None else float(wc.astype(np.float64).sum()),
                               nz=float(rf.size) if wc is None else float(np.count_nonzero(wc)))
                add(acc[f], slot[f])
        for a in acc:
            for key in keys:
                a[key] = np.asarray(a[key], dtype=np.float64)
            a["U"], a["V"] = a["U"].astype(dt).astype(np.float64), a["V"].astype(dt).astype(np.float64)
    return acc


def model_results(acc, flags, dt, weighted, items=ITEMS, mutant=None):
    """The model's outputs per item from the accumulated units (test_streaming_host.close / finish / union_update:
    G = sum_f U_f in fold order, a union's folds ascending), with one seeded defect:
      union_stats_of_wrong_fold   the statistics of a union use its first fold for every member
      union_unordered             the members are subtracted from G one at a time in descending order"""
    import test_streaming_host as model

    def pack(res):
        # (the kernels form the upper tiles and mirror them: XTX is symmetric to the bit, a BLAS product is not)
        (xtx, xty), st = res
        xtx = np.triu(xtx) + np.triu(xtx, 1).T
        return dict(zip(hc.NAMES, (xtx, xty) + tuple(st)))
    out = {}
    with np.errstate(all="ignore"):
        tot = model.close(acc, dt)
        for item in items:
            if item[0] == "fold":
                upd = acc[item[1]]
            else:
                S = sorted(item[1])
                upd = model.union_update(acc, S)
                if mutant == "union_stats_of_wrong_fold":
                    for key in ("s", "q", "sy", "qy", "sw", "nz"):
                        upd[key] = acc[S[0]][key] * float(len(S))
                elif mutant == "union_unordered" and len(S) > 1:
                    # total - upd must come out as ((G - U_last) - ...) - U_first: hand the finish a total that has
                    # all members but the first subtracted already
                    tot_u = dict(tot)
                    upd = dict(upd)
                    for key in ("U", "V"):
                        t = tot[key]
                        for f in S[:0:-1]:
                            t = t - acc[f][key]
                        tot_u[key], upd[key] = t, acc[S[0]][key]
                    out[item] = pack(model.finish(tot_u, upd, flags, "XTX_XTY", 1, dt, weighted, True))
                    continue
            out[item] = pack(model.finish(tot, upd, flags, "XTX_XTY", 1, dt, weighted, True))
    return out


def model_run(X, Y, w, chunking, flags, dt, items=ITEMS, mutant=None, labels=None, rows=None):
    labels = design()[0] if labels is None else labels
    rows = chunk_rows(chunking, labels, w) if rows is None else rows
    acc = model_accumulate(X, Y, w, labels, rows, dt, mutant)
    return model_results(acc, flags, dt, w is not None, items, mutant)
