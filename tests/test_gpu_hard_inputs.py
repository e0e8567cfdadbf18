"""GPU (-m gpu): the fold stage on the inputs the rest of the suite never draws -- a NaN, an Inf or an overflowing
cell in X, Y or the weights; columns whose mean is far from zero, so that subtract-and-correct cancels; column and
weight scales spread over many decades.  Cases and helpers: tests/hard_input_cases.py; tests/test_hard_inputs_oracle.py
checks on the CPU that every case means something for the oracle alone.

Containment: the non-finite mask of every output of every fold of the batch is the NumPy oracle's, element for element
(a zero weight does not hide a NaN: 0 * NaN is NaN; a zero operand of a padded or clamped load does not spread one),
the finite entries meet the suite's gates, XTX is symmetric, and ``fold_status()`` stays 0.

What containment can and cannot see: the training matrices are the full-data matrices minus the fold's, so a NaN in
column c of any row already poisons column c of every fold.  A loader that lets a neighbouring row in under weight 0
therefore changes no mask (tried on a scratch copy of the mid-tile kernel: padded rows read from the previous fold's
rows, every containment case still passes, and on finite data the leak adds 0); what these cases catch is a NaN that
crosses columns, reaches XTX from Y, is lost, or sets the status.  The row positions are there so that each loader
path (first stage, partial stage, absent row, short block) carries the NaN once.

Cancellation ladder: err(product vs exact) <= 2 err(oracle in the same element type vs exact) + floor (BASELINE.md
section 4, cvmatrix_amd/fp32_gate.py; floor 1e-10 in float64), exact being the definition in extended precision.

The yardstick is the largest oracle error over three fixed row orders of the same problem (as given, reversed, a
seeded shuffle; hc.row_orders), not the error of the rows as given alone.  With the single order one comparison stood
above 2: tile shape, eager fit, offset 1e4, weighted, fold 1, sdY (three entries) at 8.4e-8 against 2.7e-8, ratio 3.10.
The kernel is honest there -- the same output of the same fold stands at 0.10, 0.06 and 0.06 of the yardstick on the
rungs 1, 1e2 and 1e6, and the lazy fit at 0.86 on this one, so no term is missing and nothing grows with the rung --
and the oracle's own error on the reversed and shuffled rows is 3.2e-7 and 2.6e-7: 2.7e-8 was a lucky draw of a
cancelling sum of three entries.  The factor stays 2.

Observed on an MI355X (CVM_HARD_REPORT=path writes one line per comparison: fit mode, route, offset, run, fold, output,
err, oracle err on the rows as given, yardstick, ratio): the largest err / yardstick over both fit modes, the three
runs, the checked folds and the six outputs, among the comparisons whose error is above the floor (below it the ratio
says nothing; on the first float64 rung, and on the small-fold route at 1e2, every error is below 1e-10); in brackets
the same against the single-order oracle error.

    route          rung 1        rung 2        rung 3        rung 4
    tile_f64       -             0.17 (0.22)   0.26 (3.10)   0.19 (0.27)
    fused_f64      -             0.27 (0.27)   0.40 (0.43)   0.37 (0.67)
    mid_f64        -             0.44 (0.45)   0.58 (0.58)   0.57 (0.57)
    small_f64      -             -             0.37 (0.56)   0.27 (0.56)
    tile_f32_dma   0.10 (0.13)   0.11 (0.11)   0.10 (0.11)   0.12 (0.13)
    resident_f32   0.63 (0.75)   0.92 (0.96)   0.87 (0.87)   0.72 (0.89)

(rungs: offsets 1, 1e2, 1e4, 1e6 in float64; 1, 3, 10, 30 in float32.)  No ratio grows with the rung.  Where the yardstick itself is
above 0.1 the oracle has no result left and twice it bounds nothing: those comparisons are not made (XTY on the top
float64 rung of the tile and fused shapes, hc.LADDER_BEYOND, held to exactly that list on the CPU); XTX and the
statistics of those rungs are compared like the rest.  The resident
route sums in the oracle's element type with ``sqrt(sw) mu`` operands and sits nearest to the oracle's own error; the
LDS-DMA tile route keeps float64 partial sums and sits a factor ten below it.

Scale spread, statistics: a mean of signed values under weights spread over six decades (some twenty effective rows)
can be hundreds of times smaller than the column it averages; the float32 means are held to 2e-6 of the larger of
|mean| and sum(w |x|) / sum(w) (hc.mean_scales), which is |mean| wherever the values share a sign.  The oracle's own
float32 run is off by up to 2.5e-5 of such a mean and 1e-6 of that scale.  float64 keeps the element-wise 1e-10.
"""

import os

import numpy as np
import pytest

import hard_input_cases as hc
from conftest import to_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["lazy_fit", "eager_fit"])
def amd(hip_device, request):
    """As in test_gpu_parity.py: every test runs with the package defaults (lazy fit, private device copies padded to
    16-byte rows) and with CVM_LAZY_FIT=0 CVM_PAD=0 (fit kernel, then the fold kernels on the caller's shapes)."""
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


def _product(amd, style, X, Y, w, folds, flags, dtype, backend="hip"):
    """The product's outputs for every fold (a list of name -> array or None, like hc.oracle_fold_results) through the
    call that takes the route, and the model."""
    m = amd.CVMatrix(*flags, ddof=1, dtype=dtype, backend=backend)
    if style == "sweep":
        labels = np.empty(X.shape[0], dtype=np.int64)
        for k, v in enumerate(folds):
            labels[v] = k
        m.fit(X, Y, w, folds=amd.Partitioner(labels))
        assert m.sweep_folds is not None and m.sweep_folds.is_partition
        (bx, by), st = m.training_XTX_XTY_batched(m.sweep_folds)
    elif style == "stats":
        m.fit(X, Y, w)
        bx = by = None
        st = m.training_statistics_batched(folds)
    elif style == "resident":
        from cvmatrix_amd import _lib

        lib = _lib.load()
        assert lib.cvm_debug_resident(1) == 0
        try:
            m.fit(X, Y, w)
            (bx, by), st = m.training_XTX_XTY_batched(folds)
            bx, by = to_np(bx), to_np(by)
        finally:
            lib.cvm_debug_resident(2)
    else:
        m.fit(X, Y, w)
        (bx, by), st = m.training_XTX_XTY_batched(folds)
    arrs = [None if a is None else to_np(a) for a in (bx, by) + tuple(st)]
    if backend == "numpy":
        assert all(a is None or isinstance(a, np.ndarray) for a in (bx, by) + tuple(st))
    return [dict(zip(hc.NAMES, (None if a is None else a[f] for a in arrs))) for f in range(len(folds))], m


def _containment(amd, route, case):
    dtype, N, K, M, folds, style, rows = hc.route_geometry(route)
    kind, flags, rn, col = case
    X, Y, w = hc.poisoned(*hc.route_problem(route), kind, rows[rn], col)
    stats_only = style == "stats"
    ref = hc.oracle_fold_results(X, Y, w, folds, flags, stats_only=stats_only)
    ref32 = hc.oracle_fold_results(X, Y, w, folds, flags, dtype=np.float32, stats_only=stats_only) if dtype is np.float32 else None
    got, m = _product(amd, style, X, Y, w, folds, flags, dtype)
    assert len(got) == len(folds)
    for f in range(len(folds)):
        hc.compare_fold(got[f], ref[f], None if ref32 is None else ref32[f], kind, col, dtype, f"{route} {hc.case_id(case)} fold{f}")
    assert m.fold_status() == 0          # a NaN that comes from the data is no fault of the fold stage
    if case == hc.containment_cases(route)[0]:
        _product(amd, style, X, Y, w, folds, flags, dtype, backend="numpy")     # arrays, no raise


def _cases(route):
    return pytest.mark.parametrize("case", hc.containment_cases(route), ids=hc.case_id)


@_cases("tile_f64")
def test_containment_tile_gram_and_finalize(amd, case):
    """Tile Gram + finalize over several row splits, float64: folds of 300 / 1 / 0 / 349 / 50 rows at K = 130."""
    _containment(amd, "tile_f64", case)


@_cases("tile_f64_odd_k")
def test_containment_tile_gram_odd_k(amd, case):
    """K = 129: the general kernel's scalar loads (eager fit, unpadded), or the padded copy with the poisoned last
    column next to the padding (lazy fit)."""
    _containment(amd, "tile_f64_odd_k", case)


@_cases("tile_f32_dma")
def test_containment_float32_lds_dma(amd, case):
    _containment(amd, "tile_f32_dma", case)


@_cases("sweep_f64")
def test_containment_one_sweep_fit(amd, case):
    """fit(folds=partition): the full-data matrices are the sum of the folds' validation matrices."""
    _containment(amd, "sweep_f64", case)


@_cases("fused_f64")
def test_containment_fused_epilogue_float64(amd, case):
    _containment(amd, "fused_f64", case)


@_cases("fused_f32")
def test_containment_fused_epilogue_float32(amd, case):
    _containment(amd, "fused_f32", case)


@_cases("mid_f64")
def test_containment_mid_tile_float64(amd, case):
    _containment(amd, "mid_f64", case)


@_cases("mid_f32")
def test_containment_mid_tile_float32(amd, case):
    _containment(amd, "mid_f32", case)


@_cases("small_f64")
def test_containment_direct_small_folds(amd, case):
    _containment(amd, "small_f64", case)


@_cases("loo_rows_f64")
def test_containment_leave_one_out_rows_kernel(amd, case):
    _containment(amd, "loo_rows_f64", case)


@_cases("resident_f32")
def test_containment_resident_float32(amd, case):
    _containment(amd, "resident_f32", case)


@_cases("resident_f32_36")
def test_containment_resident_float32_blocks_of_36_rows(amd, case):
    _containment(amd, "resident_f32_36", case)


@_cases("stats_f64")
def test_containment_statistics_kernel(amd, case):
    _containment(amd, "stats_f64", case)


@pytest.mark.parametrize("zero_weight", [False, True])
def test_validation_sse_keeps_a_nan_in_its_own_fold(amd, zero_weight):
    """pls_validation_sse with a NaN in one validation row of fold 1 (once with that row's weight 0: 0 * NaN is NaN):
    sse[1] is all NaN, sse[0] and sse[2] are the torch formula's (tests/test_gpu_pls.py::test_validation_sse_on_the_device)
    to its 1e-10; statistics of the clean model, coefficients finite and random."""
    import torch

    from cvmatrix_amd.pls import pls_validation_sse

    rng = np.random.default_rng(936)
    N, K, M, P, A = 900, 36, 4, 3, 5
    X = rng.standard_normal((N, K)) + 0.5
    Y = rng.standard_normal((N, M))
    w = rng.random(N) + 0.1
    labels = np.arange(N) % P
    row = int(np.flatnonzero(labels == 1)[7])
    Xp = X.copy()
    Xp[row, 5] = np.nan
    if zero_weight:
        w[row] = 0
    part = amd.Partitioner(labels)
    clean = amd.CVMatrix()
    clean.fit(X, Y, w)
    _, stats = clean.training_XTX_XTY_batched(part)
    cvm = amd.CVMatrix()
    cvm.fit(Xp, Y, w)
    batch = cvm.prepare_folds(part)
    B = torch.from_numpy(rng.standard_normal((P, A, K, M))).to(stats[0].device)
    sse, wsum = pls_validation_sse(cvm, batch, stats, B)
    muX, sdX, muY, sdY = stats
    for f, key in enumerate(part.folds_dict):
        val = torch.from_numpy(part.get_validation_indices(key)).to(B.device)
        pred = torch.matmul((cvm.X[val] - muX[f]) / sdX[f], B[f]) * sdY[f] + muY[f]
        ref = ((pred - cvm.Y[val]) ** 2 * cvm.weights[val]).sum(dim=1)
        if f == 1:
            assert bool(torch.isnan(ref).all()) and bool(torch.isnan(sse[f]).all())
        else:
            assert bool(torch.isfinite(sse[f]).all())
            assert float((sse[f] - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    assert bool(torch.isfinite(wsum).all())


# ---------------------------------------------------------------------------------------- cancellation ladder
def _ladder_params():
    out = []
    for route, (base, _, _) in hc.LADDER_ROUTES.items():
        for off in hc.LADDER[hc.ROUTES[base][0]]:
            for run, _, _ in hc.LADDER_RUNS:
                out.append(pytest.param(route, off, run, id=f"{route}-{off:g}-{run}"))
    return out


@pytest.mark.parametrize("route,off,run", _ladder_params())
def test_cancellation_ladder(amd, route, off, run):
    base = hc.LADDER_ROUTES[route][0]
    dtype, style = hc.ROUTES[base][0], hc.ROUTES[base][5]
    flags, weighted = next((fl, wt) for n, fl, wt in hc.LADDER_RUNS if n == run)
    X, Y, w, folds, checked = hc.ladder_problem(route, off)
    reference = hc.ladder_reference(route, off, run)
    got, m = _product(amd, style, X, Y, w if weighted else None, folds, flags, dtype)
    cols, floor = hc.ladder_columns(route), hc.ladder_floor(dtype)
    bad = []
    for f in checked:
        exact, as_given, yard = reference[f]
        g = hc.cut_columns(got[f], cols)
        for n, y in yard.items():
            assert np.isfinite(g[n]).all(), (route, off, run, f, n)
            if y > hc.LADDER_MAX_YARD:          # no longer a result in the oracle (hc.LADDER_BEYOND lists where)
                assert (route, off, n) in hc.LADDER_BEYOND
                continue
            err = hc.nerr(g[n], exact[n])
            hc.report(f"{os.environ['CVM_LAZY_FIT']}\t{route}\t{off:g}\t{run}\tfold{f}\t{n}\t{err:.3e}\t{as_given[n]:.3e}\t{y:.3e}\t"
                      f"{err / max(y, 1e-300):.2f}")
            if not err <= 2 * y + floor:
                bad.append((f, n, err, y))
    assert not bad, f"{route} offset {off:g} {run}: error above 2 x the oracle's own + {floor:.1e}; (fold, output, err, oracle err): {bad}"
    assert m.fold_status() == 0


# ---------------------------------------------------------------------------------------- scale spread
def _spread_params():
    return [pytest.param(dtype, span, wspan, route, id=f"{route}-span{span}-{dtype.__name__}")
            for dtype, span, wspan in hc.SPREADS for route in hc.SPREAD_ROUTES[dtype]]


@pytest.mark.parametrize("dtype,span,wspan,route", _spread_params())
def test_column_and_weight_scales_spread_over_decades(amd, dtype, span, wspan, route):
    """All flags on: scaling normalises every column, the suite's gates apply unchanged to the scaled outputs.  float64
    with scaling off: every (decade, decade) block of XTX against its own max, so that a column of 1e-6 next to one
    of 1e6 is seen."""
    style = hc.ROUTES[route][5]
    X, Y, w, folds, ex = hc.spread_case(route, span, wspan, dtype)
    ref = hc.oracle_fold_results(X, Y, w, folds, hc.ON)
    ref32 = hc.oracle_fold_results(X, Y, w, folds, hc.ON, dtype=np.float32) if dtype is np.float32 else None
    got, m = _product(amd, style, X, Y, w, folds, hc.ON, dtype)
    for f in range(len(folds)):
        scales = hc.mean_scales(X, Y, w, folds[f]) if dtype is np.float32 else {}
        for n in hc.NAMES:
            if n in hc.STAT_NAMES:
                gate = hc.gate_stats(hc.STAT_RTOL[dtype], scale=scales.get(n))
            else:
                gate = hc.gate_float64() if dtype is np.float64 else hc.gate_float32(ref32[f][n])
            hc.assert_matches_oracle_where_finite(np.reshape(got[f][n], np.shape(ref[f][n])), ref[f][n], gate,
                                                  f"{route} span {span} fold{f} {n}")
    assert m.fold_status() == 0
    if dtype is np.float64:
        groups = hc.decade_groups(ex)
        ref = hc.oracle_fold_results(X, Y, w, folds, hc.CENTRE_ONLY)
        got, m = _product(amd, style, X, Y, w, folds, hc.CENTRE_ONLY, dtype)
        for f in range(len(folds)):
            hc.assert_blockwise(got[f]["XTX"], ref[f]["XTX"], groups, what=f"{route} span {span} fold{f} XTX")
