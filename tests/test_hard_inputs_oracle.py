"""CPU: the cases of tests/test_gpu_hard_inputs.py meet their own conditions for the oracle alone -- the
non-finite mask of every containment case is the stated one (and the comparison is not vacuous), every
rung of the cancellation ladder leaves the oracle an error that is still a result and (from the second
rung on) is cancellation and not the floor, and the scale-spread problems leave the oracle at rounding."""

import numpy as np
import pytest

import hard_input_cases as hc


@pytest.mark.parametrize("route", list(hc.ROUTES))
def test_containment_cases_have_the_stated_oracle_mask(route):
    dtype, N, K, M, folds, style, rows = hc.route_geometry(route)
    X, Y, w = hc.route_problem(route)
    cases = hc.containment_cases(route)
    stats_only = style == "stats"
    # every column position and every row position at least once per route
    assert {c[3] for c in cases} == set(hc.route_columns(K))
    assert {c[2] for c in cases} == set(rows)
    assert len(set(rows.values())) == len(rows)
    if style == "sweep":
        assert np.array_equal(np.sort(np.concatenate(folds)), np.arange(N))
    for r in rows.values():
        assert w[r] > 0
    for case in cases:
        kind, flags, rn, col = case
        Xp, Yp, wp = hc.poisoned(X, Y, w, kind, rows[rn], col)
        ref = hc.oracle_fold_results(Xp, Yp, wp, folds, flags, stats_only=stats_only)
        want = hc.expected_masks(kind, flags, K, M, col, stats_only)
        for f, r in enumerate(ref):
            hc.refuse_vacuous(kind, r, K)
            for n in hc.NAMES:
                assert (r[n] is None) == (want[n] is None), (hc.case_id(case), f, n)
                if r[n] is not None:
                    assert np.array_equal(~np.isfinite(r[n]), want[n]), (hc.case_id(case), f, n)
        if dtype is np.float32:             # the float32 yardstick run has the same mask
            r32 = hc.oracle_fold_results(Xp, Yp, wp, folds[:2], flags, dtype=np.float32, stats_only=stats_only)
            for n in hc.NAMES:
                if want[n] is not None:
                    assert np.array_equal(~np.isfinite(r32[0][n]), want[n]), (hc.case_id(case), n)


def test_the_helper_sees_a_leak_a_lost_nan_and_a_wrong_number():
    ref = np.arange(16.0).reshape(4, 4)
    ref[1, :] = ref[:, 1] = np.nan
    gate = hc.gate_float64()
    hc.assert_matches_oracle_where_finite(ref.copy(), ref, gate)
    for i, j, v in ((2, 2, np.nan), (1, 2, 0.0), (3, 3, 15.0 * (1 + 1e-9))):
        got = ref.copy()
        got[i, j] = v
        with pytest.raises(AssertionError):
            hc.assert_matches_oracle_where_finite(got, ref, gate)
    with pytest.raises(AssertionError):     # nothing poisoned: refused
        hc.refuse_vacuous("nan_x", {"XTX": np.ones((4, 4))}, 4)
    with pytest.raises(AssertionError):     # too little left finite: refused
        hc.refuse_vacuous("nan_x", {"XTX": np.full((4, 4), np.nan)}, 4)
    # statistics: element-wise, an entry far below its scale against the scale
    st = np.array([[2.0, 1e-3, np.nan]])
    hc.assert_matches_oracle_where_finite(st * [1, 1 + 1e-6, 1], st, hc.gate_stats(2e-6))
    hc.assert_matches_oracle_where_finite(st + [0, 1e-6, 0], st, hc.gate_stats(2e-6, scale=[2.0, 1.0, 1.0]))
    for got, g in ((st * [1, 1 + 1e-5, 1], hc.gate_stats(2e-6)), (st + [0, 1e-6, 0], hc.gate_stats(2e-6)),
                   (st + [0, 1e-5, 0], hc.gate_stats(2e-6, scale=[2.0, 1.0, 1.0])), (st * [np.nan, 1, 1], hc.gate_stats(2e-6))):
        with pytest.raises(AssertionError):
            hc.assert_matches_oracle_where_finite(got, st, g)
    # overflow: the rest of the matrix is compared against its own max, not against 1e200
    big = np.ones((4, 4))
    big[1, :] = big[:, 1] = 1e200
    off = big.copy()
    off[2, 2] = 1.0 + 1e-6
    hc.assert_matches_oracle_where_finite(off, big, gate)
    with pytest.raises(AssertionError):
        hc.assert_matches_oracle_where_finite(off, big, gate, blocks=hc.overflow_blocks((4, 4), 1))


@pytest.mark.parametrize("route", list(hc.LADDER_ROUTES))
def test_ladder_rungs_are_meaningful_for_the_oracle(route):
    """The band of every rung, on the yardstick the GPU gate uses (the largest oracle error over the three row orders):
    at most 0.1 (still a result), and from the second rung on at least 1e-10 / 1e-5 in the matrices on the rows as
    given (cancellation, not the floor).  The comparisons beyond the band are not made on the GPU; hc.LADDER_BEYOND
    names every (route, offset, output) that has one and no other, so the list cannot grow unnoticed."""
    dtype = hc.ROUTES[hc.LADDER_ROUTES[route][0]][0]
    beyond = set()
    for i, off in enumerate(hc.LADDER[dtype]):
        for run, flags, weighted in hc.LADDER_RUNS:
            for f, (exact, as_given, yard) in hc.ladder_reference(route, off, run).items():
                beyond |= {(route, off, n) for n, y in yard.items() if not y <= hc.LADDER_MAX_YARD}
                assert all(as_given[n] <= y for n, y in yard.items())
                if i >= 1 and flags == hc.ON:
                    assert max(as_given["XTX"], as_given["XTY"]) >= hc.LADDER_MIN_ERR[dtype], (route, off, run, f, as_given)
    assert beyond == {b for b in hc.LADDER_BEYOND if b[0] == route}, beyond


@pytest.mark.parametrize("dtype,span,wspan", hc.SPREADS)
def test_spread_problems_leave_the_oracle_at_rounding(dtype, span, wspan):
    needed = False
    for route in hc.SPREAD_ROUTES[dtype]:
        X, Y, w, folds, ex = hc.spread_case(route, span, wspan, dtype)
        assert X.dtype == dtype
        for flags in (hc.ON,) + ((hc.CENTRE_ONLY,) if dtype is np.float64 else ()):
            orc = hc.oracle_fold_results(X, Y, w, folds, flags, dtype=dtype)
            for f, o in enumerate(orc):
                exact = hc.exact_training_matrices(X, Y, w, folds[f], flags)
                if flags == hc.ON:
                    for n in hc.NAMES:
                        assert hc.nerr(o[n], exact[n]) <= hc.SPREAD_MAX_ERR[dtype], (route, f, n, hc.nerr(o[n], exact[n]))
                else:       # scaling off: block by block, or only the largest columns are seen
                    groups = hc.decade_groups(ex)
                    assert len(groups) >= 2
                    assert hc.blockwise_errors(o["XTX"], exact["XTX"], groups).max() <= hc.SPREAD_MAX_ERR[dtype], (route, f)
        if dtype is np.float32:
            # the means: the oracle's own float32 run against its float64 run meets the rule of the GPU test (2e-6 of
            # the larger of |mean| and sum(w |x|) / sum(w)) on every fold
            ref = hc.oracle_fold_results(X, Y, w, folds, hc.ON)
            o32 = hc.oracle_fold_results(X, Y, w, folds, hc.ON, dtype=np.float32)
            for f in range(len(folds)):
                scales = hc.mean_scales(X, Y, w, folds[f])
                for n in ("muX", "muY"):
                    hc.assert_matches_oracle_where_finite(o32[f][n], ref[f][n], hc.gate_stats(hc.STAT_RTOL[dtype], scale=scales[n]),
                                                          f"{route} fold{f} {n}")
                    rel = np.abs(o32[f][n].astype(np.float64) - ref[f][n]) / np.abs(ref[f][n])
                    needed |= bool(rel.max() > 5 * hc.STAT_RTOL[dtype])
    if dtype is np.float32:
        # ... and misses the element-wise 2e-6 by more than five times somewhere: that rule cannot be asked of a
        # float32 sum on these inputs, which is why the GPU test scales the means
        assert needed
