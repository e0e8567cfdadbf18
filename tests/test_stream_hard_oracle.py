"""CPU: the cases of tests/test_gpu_stream_hard.py meet their own conditions for the oracle alone -- every containment
case is poisoned somewhere and keeps (K - 1)^2 entries of XTX finite for every fold and union, with the poisoned row
where its name says and the poisoned fold inside a union, outside one and a union of its own; every rung of the ladder
leaves the oracle a result (or is on shc.LADDER_BEYOND, held to exactly what the oracle yields) that from the second
rung on is cancellation and not the floor; the spread problems leave the oracle at rounding -- and the tests have
teeth: a NumPy model of the streaming sums and of the union sums passes the assertion functions the GPU test calls, and
with one seeded defect (shc.MUTANTS) fails at least one case of them."""

import numpy as np
import pytest

import hard_input_cases as hc
import stream_hard_cases as shc
import unions_cases as uc


def test_design_and_chunkings():
    labels, folds = shc.design()
    assert tuple(len(f) for f in folds) == uc.SIZES and len(labels) == uc.N
    rest = lambda item: uc.N - len(shc.validation_rows(item))      # noqa: E731
    assert tuple(rest(i) for i in shc.UNION_ITEMS) == shc.COMPLEMENT_ROWS and rest(shc.SMALLEST) == 22
    w = shc.clean_problem(shc.K, shc.M, "float64")[2]
    for name in ("B", "C", "S", "W"):
        rows = shc.chunk_rows(name, labels, w)
        assert sorted(np.concatenate(rows).tolist()) == list(range(uc.N)), name
    assert [len(r) for r in shc.chunk_rows("S", labels)] == [16] * 12 + [11]
    chunks = shc.chunk_rows("W", labels, w)
    assert len(chunks) == 8 and all(w[a].max() <= w[b].min() for a, b in zip(chunks[:-1], chunks[1:]))
    # the weights: a tenth zero, no fold all zero, none of the poison rows
    assert int((w == 0).sum()) == uc.N // 10 and all((w[f] > 0).any() for f in folds)
    pr = shc.poison_rows()
    for r, _ in pr.values():
        for q in np.atleast_1d(r):
            assert w[q] > 0 and w[hc.pair_row(int(q), uc.N)] > 0
    # the row positions are what their names say
    B, C, S = (shc.chunk_rows(n, labels) for n in ("B", "C", "S"))
    assert B[2].tolist() == [pr["one_row"][0]] and pr["one_row"][1] == "B"
    assert any(r[0] == pr["chunk_first"][0] for r in S[1:])
    assert S[-1][-1] == pr["last_partial"][0] and len(S[-1]) % 16
    assert sum(pr["lone_fold"][0] in r for r in C) == 1 and all(len(set(labels[r])) == 1 for r in C)
    (a, b), _ = pr["pair_same_fold"]
    assert a in B[0] and b in B[-1] and labels[a] == labels[b]
    (a, b), _ = pr["pair_two_folds"]
    assert a in S[0] and b in S[-1] and labels[a] != labels[b]


@pytest.mark.parametrize("k,m", [(shc.K, shc.M), shc.SMALL])
@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_containment_cases_mean_something_for_the_oracle(k, m, dtype):
    name = np.dtype(dtype).name
    cases = shc.containment_cases(k, dtype)
    kinds = {c[0] for c in cases}
    assert kinds == set(hc.KINDS) - (set() if dtype is np.float64 else {"overflow_x"})
    assert {c[3] for c in cases} == set(hc.route_columns(k))
    assert {c[2] for c in cases} == set(shc.poison_rows())
    assert all(c[2] == "one_row" for c in cases if c[0] == "nan_x_zero_w")
    for kind in kinds - {"nan_w", "overflow_x"}:
        assert {c[1] for c in cases if c[0] == kind} == {hc.ON, hc.OFF}
    for case in cases:
        kind, flags, rn, col = case
        X, Y, w, ref, ref32, st, st32 = shc.containment_reference(k, m, name, case)
        assert X.dtype == dtype
        f = shc.case_fold(case)
        unions = [i[1] for i in shc.case_items(case) if i[0] == "union"]
        assert (f,) in unions and any(f in S and len(S) > 1 for S in unions) and any(f not in S for S in unions)
        for item in shc.case_items(case):
            hc.refuse_vacuous(kind, ref[item], k)
            if ref32 is not None:               # the float32 yardstick run has the same mask
                for nm in hc.NAMES:
                    assert (ref[item][nm] is None) == (ref32[item][nm] is None)
                    if ref[item][nm] is not None:
                        assert np.array_equal(np.isfinite(ref[item][nm]), np.isfinite(ref32[item][nm])), (shc.case_id(case), item, nm)
        if st is not None:
            for r in st:
                hc.refuse_vacuous(kind, r, k)
        # a mask that matters: apart from a NaN weight the case leaves finite entries in every output it poisons
        if kind in hc.X_KINDS and not rn.startswith("pair_"):
            want = hc.expected_masks(kind, flags, k, m, col)
            for item in shc.case_items(case):
                for nm in hc.NAMES:
                    assert (ref[item][nm] is None) == (want[nm] is None)
                    if want[nm] is not None:
                        assert np.array_equal(~np.isfinite(ref[item][nm]), want[nm]), (shc.case_id(case), item, nm)


@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_ladder_rungs_are_meaningful_for_the_oracle(dtype):
    """The yardstick of every comparison is at most hc.LADDER_MAX_YARD or the comparison is on shc.LADDER_BEYOND, which
    holds exactly those; from the second rung on the oracle's error in XTX or XTY on the rows as given is above
    hc.LADDER_MIN_ERR (the runs of hc.LADDER_RUNS with every flag on; the drift run spreads the columns and is there
    for its chunk means).  No yardstick of the forced-split rung is beyond."""
    name = np.dtype(dtype).name
    beyond = set()
    top = hc.LADDER[dtype][-1]
    for i, off in enumerate(hc.LADDER[dtype]):
        for run in shc.ladder_runs():
            flags = shc.run_settings(run)[0]
            for item, (exact, as_given, yard) in shc.ladder_reference(name, off, run).items():
                beyond |= {(name, off, shc.item_id(item), nm) for nm, y in yard.items() if not y <= hc.LADDER_MAX_YARD}
                assert all(as_given[nm] <= y for nm, y in yard.items())
                if i >= 1 and flags == hc.ON and run != shc.DRIFT:
                    assert max(as_given["XTX"], as_given["XTY"]) >= hc.LADDER_MIN_ERR[dtype], (off, run, item, as_given)
    assert beyond == {b for b in shc.LADDER_BEYOND if b[0] == name}, beyond
    for _, off, item, nm in beyond:
        assert nm in ("XTX", "XTY") and off == top and item == shc.item_id(shc.SMALLEST)
    reference = shc.split_problem(name)[-1]
    assert set(reference) == set(shc.SPLIT_ITEMS)
    for item, (exact, as_given, yard) in reference.items():
        assert all(y <= hc.LADDER_MAX_YARD for y in yard.values()), (item, yard)
        assert max(as_given["XTX"], as_given["XTY"]) >= hc.LADDER_MIN_ERR[dtype]


def test_the_beyond_list_keeps_its_condition():
    tops = {np.dtype(dt).name: hc.LADDER[dt][-1] for dt in shc.DTYPES}
    for name, off, item, nm in shc.LADDER_BEYOND:
        assert nm in ("XTX", "XTY") and off == tops[name] and item == shc.item_id(shc.SMALLEST)


@pytest.mark.parametrize("dtype,span,wspan", hc.SPREADS)
def test_spread_problems_leave_the_oracle_at_rounding(dtype, span, wspan):
    X, Y, w, groups, refs, scales = shc.spread_reference(np.dtype(dtype).name, span, wspan)
    assert X.dtype == dtype and len(groups) >= 2
    for flags in (hc.ON, hc.CENTRE_ONLY):
        orc = shc.oracle_items(X, Y, w, flags, dtype)
        for item in shc.ITEMS:
            exact = hc.exact_training_matrices(X, Y, w, shc.validation_rows(item), flags)
            if flags == hc.ON:
                for nm in hc.NAMES:
                    assert hc.nerr(orc[item][nm], exact[nm]) <= hc.SPREAD_MAX_ERR[dtype], (item, nm, hc.nerr(orc[item][nm], exact[nm]))
            else:
                assert hc.blockwise_errors(orc[item]["XTX"], exact["XTX"], groups).max() <= hc.SPREAD_MAX_ERR[dtype], item


# ---------------------------------------------------------------------------------------- the tests have teeth
def _containment_runs(mutant, dtypes=shc.DTYPES):
    """(what, a call that raises AssertionError where the model with ``mutant`` misses the containment assertion)."""
    for dtype in dtypes:
        name = np.dtype(dtype).name
        for case in shc.containment_cases(shc.K, dtype):
            def run(case=case, dtype=dtype, name=name):
                reference = shc.containment_reference(shc.K, shc.M, name, case)
                X, Y, w = reference[:3]
                got = shc.model_run(X, Y, w, shc.case_chunking(case), case[1], dtype, shc.case_items(case), mutant)
                shc.assert_containment(got, reference, case, dtype, "model")
            yield f"containment {name} {shc.case_id(case)}", run


def _ladder_runs(mutant, dtypes=shc.DTYPES, rungs=(1, 3), runs=("weighted", shc.DRIFT), chunkings=shc.LADDER_CHUNKINGS):
    for dtype in dtypes:
        name = np.dtype(dtype).name
        for off in (hc.LADDER[dtype][i] for i in rungs):
            for run_name in runs:
                for chunking in chunkings:
                    def run(dtype=dtype, name=name, off=off, run_name=run_name, chunking=chunking):
                        X, Y, w = shc.ladder_problem(name, off, run_name)
                        got = shc.model_run(X, Y, w, chunking, shc.run_settings(run_name)[0], dtype, shc.ITEMS, mutant)
                        shc.assert_ladder(got, shc.ladder_reference(name, off, run_name), dtype, off, run_name, f"model-{chunking}")
                    yield f"ladder {name} {off:g} {run_name} {chunking}", run


def _spread_runs(mutant):
    for dtype, span, wspan in hc.SPREADS:
        for flags in (hc.ON, hc.CENTRE_ONLY):
            for chunking in shc.SPREAD_CHUNKINGS:
                def run(dtype=dtype, span=span, wspan=wspan, flags=flags, chunking=chunking):
                    reference = shc.spread_reference(np.dtype(dtype).name, span, wspan)
                    X, Y, w = reference[:3]
                    got = shc.model_run(X, Y, w, chunking, flags, dtype, shc.ITEMS, mutant)
                    shc.assert_spread(got, reference, flags, dtype, f"model-{chunking}")
                yield f"spread {dtype.__name__} span {span} {'on' if flags == hc.ON else 'centre'} {chunking}", run


def _failures(runs):
    failed, n = [], 0
    for what, run in runs:
        n += 1
        try:
            run()
        except (AssertionError, ValueError):      # (ValueError: the model's finish refuses the counts it was handed)
            failed.append(what)
    return failed, n


def test_the_model_without_a_defect_passes_every_assertion(monkeypatch):
    monkeypatch.delenv("CVM_HARD_REPORT", raising=False)
    for runs in (_containment_runs(None), _ladder_runs(None, rungs=(0, 1, 2, 3), runs=shc.ladder_runs()), _spread_runs(None)):
        failed, n = _failures(runs)
        assert n and not failed, failed


@pytest.mark.parametrize("mutant", shc.MUTANTS)
def test_a_seeded_defect_fails_an_assertion(mutant, monkeypatch):
    """Where each defect is seen (on the machine this was written on; what is asserted is one failing case per defect).
    ``stale_slot`` and ``union_stats_of_wrong_fold``: by containment, ladder and spread cases alike.  ``nan_dropped``:
    by the containment cases.  ``float32_accumulator``: by the float64 cases of all three families -- and by no
    float32 case: over at most 13 chunks of 203 rows an accumulator in float32 adds less than the float32 oracle's own
    error, which is the yardstick of every float32 gate, so these gates do not tell it from the float64 accumulator.
    ``union_unordered`` (the members subtracted from G one at a time, in descending order) differs from the documented
    order by roundings of the size of the oracle's own and fails no case: the gates do not see the order of a union's
    subtraction, and are not meant to; the bit contracts of tests/test_gpu_unions.py pin it.  Information, no failure."""
    monkeypatch.delenv("CVM_HARD_REPORT", raising=False)
    seen = {}
    for family, runs in (("containment", _containment_runs(mutant)), ("ladder", _ladder_runs(mutant)), ("spread", _spread_runs(mutant))):
        seen[family], tried = _failures(runs)
        assert tried
    n = {k: len(v) for k, v in seen.items()}
    print(mutant, n)
    if mutant == "union_unordered":
        return
    assert sum(n.values()) >= 1, mutant
    if mutant == "nan_dropped":
        assert n["containment"] >= 1              # a lost NaN is a containment matter
    if mutant in ("stale_slot", "union_stats_of_wrong_fold"):
        assert n["containment"] >= 1 and n["ladder"] >= 1 and n["spread"] >= 1, n
