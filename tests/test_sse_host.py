"""CPU: the conditions of tests/sse_cases.py, which tests/test_gpu_sse.py relies on.  A step-by-step NumPy
emulation of the scorer's arithmetic lies inside the derived gate at every shape and on the hard-value design
(the fraction is printed: run with -s); five deliberate mistakes of the kind a kernel makes -- a dropped last
row, the neighbouring response's muY / sdY, weights taken by position, the k-tail past the last whole stage of
16 left out, a reciprocal good to 2^-24 only -- each leave the gate in at least one column at every shape; the
weight sum of an unweighted fold is its row count."""

import numpy as np
import pytest

import predict_cases as pc
import sse_cases as sc

SHAPES = ((17, 3, 3, 65), (33, 9, 7, 129), (130, 13, 5, 129), (521, 33, 3, 129), (520, 45, 4, 129))
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def cases():
    """Per (dtype, shape): the design (one fold of n rows among n + 7, in shuffled order), its reference and gate."""
    pc.require_longdouble()
    out = {}
    for dtype in DTYPES:
        for K, A, M, n in SHAPES:
            rng = np.random.default_rng(100 * K + n + (dtype is np.float32))
            d = sc.design(rng, (n,), K, A, M, dtype, extra=7)
            d["fold"] = dict(rows=d["folds"][0], B=d["B"][0], stats=pc.fold_stats(d["stats"], 0))
            d["refs"] = sc.reference(d["X"], d["Y"], d["w"], **d["fold"])
            out[np.dtype(dtype).name, K] = d
    return out


def run(d, mutant=None, w="own"):
    return sc.emulate(d["X"], d["Y"], d["w"] if w == "own" else w, mutant=mutant, **d["fold"])


@pytest.mark.parametrize("K,A,M,n", SHAPES)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_emulation_is_inside_the_gate(cases, dtype, K, A, M, n):
    d = cases[dtype, K]
    sse, wsum = run(d)
    assert sse.shape == (A, M) and d["refs"][1].shape == (A, M) and (d["refs"][1] > 0).all()
    worst = sc.assert_gate(sse, wsum, d["refs"], f"emulation {dtype} K = {K} A = {A} M = {M} n = {n}")
    assert worst > 0.0                      # (the gate is not vacuous: the emulation does round)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_emulation_is_inside_the_gate_on_hard_values(dtype):
    pc.require_longdouble()
    rng = np.random.default_rng(77)
    d = sc.hard_design(rng, (65, 129), 33, 4, 5, dtype)
    refs = sc.cv_reference(d["X"], d["Y"], d["w"], d["folds"], d["B"], d["stats"])
    # what the design is for: errors a thousandth of the predictions, an offset of Y far above them, zero weights
    e = np.sqrt(np.asarray(refs[0] / refs[2][:, None, None], dtype=np.float64))
    assert (e < 5e-3 * d["stats"][3][:, None, :]).all() and (d["w"] == 0).sum() > 10
    got = [sc.emulate(d["X"], d["Y"], d["w"], v, d["B"][f], pc.fold_stats(d["stats"], f)) for f, v in enumerate(d["folds"])]
    sc.assert_gate(np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), refs, f"emulation {dtype} hard values")


# (a reciprocal good to 2^-24 is as good as float32's own rounding of z: that mutant in float64 only)
@pytest.mark.parametrize("dtype,mutant", [(t, m) for t in ("float64", "float32") for m in sc.MUTANTS
                                          if not (t == "float32" and m == "coarse_reciprocal")])
@pytest.mark.parametrize("K,A,M,n", SHAPES)
def test_every_mutant_is_outside_the_gate(cases, dtype, K, A, M, n, mutant):
    d = cases[dtype, K]
    sse, wsum = run(d, mutant)
    ratio = np.abs(sse.astype(pc.LD) - d["refs"][0]) / d["refs"][1]
    print(f"{mutant} {dtype} K = {K}: {float(ratio.max()):.3g} times the gate in its worst column, "
          f"{int((ratio > 1).sum())} of {ratio.size} columns outside")
    assert ratio.max() > 1.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wsum_of_an_unweighted_fold_is_its_row_count(cases, dtype):
    for K, A, M, n in SHAPES:
        d = cases[dtype, K]
        refs = sc.reference(d["X"], d["Y"], None, **d["fold"])
        sse, wsum = run(d, w=None)
        assert wsum == n and refs[2] == n and wsum.dtype == np.float64
        sc.assert_gate(sse, wsum, refs, f"unweighted {dtype} K = {K}", weighted=False)


def test_the_gate_demands_the_reference_itself_where_it_is_zero():
    pc.require_longdouble()
    rng = np.random.default_rng(5)
    d = sc.design(rng, (9, 0), 5, 2, 3, np.float64)
    d["w"][d["folds"][0]] = 0.0
    refs = sc.cv_reference(d["X"], d["Y"], d["w"], d["folds"], d["B"], d["stats"])
    assert (refs[0] == 0).all() and (refs[1] == 0).all() and (refs[2] == 0).all() and (refs[3] == 0).all()
    zeros = np.zeros((2, 2, 3))
    sc.assert_gate(zeros, np.zeros(2), refs, "zero weights and an empty fold")
    zeros[1, 1, 2] = 1e-300
    with pytest.raises(AssertionError):
        sc.worst_ratio(zeros, refs[0], refs[1])
