"""GPU (-m gpu): streaming cross-validation (cvm_stream_add / cvm_stream_close through StreamingCVMatrix) and the unions
of folds (cvm_sweep_unions through CVMatrix.training_*_unions and through StreamingCVMatrix.training_*_unions, which
reads the streamed state) on the inputs their own suites never draw: a NaN, an Inf or an overflowing cell in one chunk,
column offsets that make G - sum U_f cancel down to a training set of 22 of 203 rows, column and weight scales spread
over many decades.  Cases, references and the assertion functions: tests/stream_hard_cases.py (shc);
tests/test_stream_hard_oracle.py checks on the CPU that every case means something for the oracle alone and that each
assertion function catches a seeded defect of a NumPy model of the sums.

Containment: hc.compare_fold's rule -- the non-finite mask of every output is the oracle's element for element (for
streaming the oracle fitted on all rows, for a union the oracle on the concatenated indices), the finite entries meet
the suite's gates, XTX is symmetric with a symmetric mask -- for the five folds and the unions of every case, with the
poisoned row in a one-row chunk, first in a chunk, last in a chunk of 11 rows, in a fold that has rows in one chunk
only, under weight zero, and as +Inf in the first chunk with -Inf in the last.

Stale scratch: the chunk partials live in a workspace that the allocator hands back from chunk to chunk and across
reset(); a fold without rows in a chunk is skipped.  A stream fed after a poisoned one has the bits of a fresh one, and
a chunk without rows of fold 0 leaves fold 0's accumulator unit byte for byte as it was.

Cancellation ladder: err(product vs exact) <= 2 x yardstick + floor (cvmatrix_amd/fp32_gate.py;
floor 1e-10 in float64), exact being the definition in extended precision on the training rows of the fold or union,
the yardstick the oracle's largest error in the element type over hc.row_orders.  Comparisons whose yardstick is above
hc.LADDER_MAX_YARD are not made (shc.LADDER_BEYOND: XTX and XTY of the union that leaves 22 rows, top rung).

Observed on an MI355X (CVM_HARD_REPORT=path writes one line per comparison: route, element type, offset, run, item,
output, err, oracle err on the rows as given, yardstick, ratio): the largest err / yardstick over the three runs of
hc.LADDER_RUNS and the drift run, the five folds, the seven unions and the six outputs, among the comparisons whose
error is above the floor (on the first float64 rung none is).  stream-B / C / S: StreamingCVMatrix under that
chunking, folds and unions from the streamed state; unions: CVMatrix.fit(folds=...) + training_XTX_XTY_unions; splits:
the forced plan (2, 3) on 1200 rows in two chunks, one rung.

    route       float64: 1   1e2    1e4    1e6      float32: 1   3      10     30
    stream-B             -   0.28   0.67   0.51              0.13   0.13   0.15   0.13
    stream-C             -   0.50   0.67   0.51              0.17   0.17   0.22   0.18
    stream-S             -   0.35   0.67   0.51              0.07   0.08   0.09   0.07
    unions               -   0.50   0.67   0.33              0.15   0.17   0.22   0.18
    splits                          0.13                                    0.04

No ratio grows with the rung, and none needed the NumPy model of the sums as a further ordering.  The 0.67 is sdY
(three entries) of the fold of 22 rows, the same on every route.

Found by these tests and fixed: stream_accumulate_kernel added the elements of a chunk's scratch that
the Gram launch never writes -- the strictly lower 16 x 16 blocks of a diagonal tile and the spare last statistics
word -- so the accumulator held whatever the allocator's memory had held, NaN after a poisoned stream.  No result was
affected; the stale-scratch tests below failed on it.

The spread problems' seeds are chosen so that the oracle alone is at rounding for every item (shc.SPREAD_SEED_STEP).
"""

import os

import numpy as np
import pytest
import torch

import hard_input_cases as hc
import stream_hard_cases as shc
from conftest import to_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd(hip_device):
    import cvmatrix_amd
    from cvmatrix_amd import _lib
    _lib.load()
    return cvmatrix_amd


@pytest.fixture
def pad(request, monkeypatch):
    """CVM_PAD=0: the device copies keep the caller's K and M (K = 7: rows that are not 16-byte aligned, the
    fallback Gram kernel)."""
    monkeypatch.setenv("CVM_PAD", request.param)
    return request.param


def _pick(mats, stats, i):
    arrs = [None if a is None else to_np(a)[i] for a in tuple(mats) + tuple(stats)]
    return dict(zip(hc.NAMES, arrs))


def _stream(amd, X, Y, w, labels, rows, flags, dtype, n_folds=shc.P):
    scv = amd.StreamingCVMatrix(n_folds, *flags, dtype=dtype)
    for r in rows:
        scv.partial_fit(X[r], Y[r], None if w is None else w[r], labels[r])
    return scv


def _stream_items(scv, items):
    """item -> outputs from the streamed state: the folds through training_XTX_XTY_batched, the unions through
    training_XTX_XTY_unions."""
    out = {}
    fold_items = [i for i in items if i[0] == "fold"]
    union_items = [i for i in items if i[0] == "union"]
    if fold_items:
        mats, stats = scv.training_XTX_XTY_batched()
        assert mats[0].shape[0] == scv.n_folds
        for i in fold_items:
            out[i] = _pick(mats, stats, i[1])
    if union_items:
        mats, stats = scv.training_XTX_XTY_unions([list(i[1]) for i in union_items])
        for u, i in enumerate(union_items):
            out[i] = _pick(mats, stats, u)
    return out


def _stream_statistics(scv):
    st = scv.training_statistics_batched()
    return [_pick((None, None), st, f) for f in range(scv.n_folds)]


def _fitted_unions(amd, X, Y, w, folds, flags, dtype, items):
    """item -> outputs of the unions among ``items`` through CVMatrix.fit(folds=...) + training_XTX_XTY_unions."""
    part = [np.array(f) for f in folds]                      # fold position = label
    cvm = amd.CVMatrix(*flags, ddof=1, dtype=dtype)
    cvm.fit(X, Y, w, folds=part)
    union_items = [i for i in items if i[0] == "union"]
    mats, stats = cvm.training_XTX_XTY_unions(part, [list(i[1]) for i in union_items])
    return {i: _pick(mats, stats, u) for u, i in enumerate(union_items)}, cvm


# ---------------------------------------------------------------------------------------- containment
def _containment_params():
    out = []
    for (k, m), pad in ((((shc.K, shc.M)), "1"), (shc.SMALL, "0")):
        for dtype in shc.DTYPES:
            for case in shc.containment_cases(k, dtype):
                out.append(pytest.param(pad, k, m, dtype, case, id=f"K{k}-{dtype.__name__}-{shc.case_id(case)}"))
    return out


@pytest.mark.parametrize("pad,k,m,dtype,case", _containment_params(), indirect=["pad"])
def test_containment(amd, pad, k, m, dtype, case):
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    reference = shc.containment_reference(k, m, name, case)
    X, Y, w = reference[:3]
    items, flags = shc.case_items(case), case[1]
    scv = _stream(amd, X, Y, w, labels, shc.chunk_rows(shc.case_chunking(case), labels), flags, dtype)
    assert scv.N == shc.N
    shc.assert_containment(_stream_items(scv, items), reference, case, dtype, "stream")
    if flags == hc.ON:
        shc.assert_containment_statistics(_stream_statistics(scv), reference, case, dtype, "stream")
    got, cvm = _fitted_unions(amd, X, Y, w, folds, flags, dtype, items)
    shc.assert_containment(got, reference, case, dtype, "unions")
    assert cvm.fold_status() == 0          # a NaN that comes from the data is no fault of the fold stage


# ---------------------------------------------------------------------------------------- stale scratch, reset()
def _bits(scv):
    """Every tensor the object hands out, as raw bytes (NaN-proof)."""
    out = []
    for res in (scv.training_XTX_XTY_batched(), scv.training_XTX_XTY_unions([list(S) for S in shc.UNIONS])):
        mats, stats = res
        out += [t.contiguous().view(torch.uint8).clone() for t in tuple(mats) + tuple(stats) if t is not None]
    return out


def _accumulator_is_finite(scv):
    torch.cuda.synchronize()
    return bool(torch.isfinite(scv._acc.view(torch.float64)).all())


def _nonfinite_places(scv):
    """Where the accumulator holds non-finite values, for a failure message: (fold, region, tile, the 16 x 16 blocks)."""
    from cvmatrix_amd.streaming import _unit_layout
    torch.cuda.synchronize()
    unit, stat0, Kp, Mp = _unit_layout(scv._cv._Kd, scv._cv._Md or 0)
    nt = Kp // 128 * (Kp // 128 + 1) // 2
    words = scv._acc.cpu().numpy().view(np.float64)
    out = []
    for f in range(scv.n_folds):
        u = words[f * unit // 8:(f + 1) * unit // 8]
        tiles = u[:nt * 128 * 128].reshape(nt, 128, 128)
        for t in range(nt):
            bad = np.argwhere(~np.isfinite(tiles[t]))
            if len(bad):
                out.append((f, "tile", t, sorted({(int(r) // 16, int(c) // 16) for r, c in bad})[:8], len(bad)))
        rest = np.flatnonzero(~np.isfinite(u[nt * 128 * 128:]))
        if len(rest):
            out.append((f, "panels or statistics, word", int(rest[0]) + nt * 128 * 128, "statistics from", stat0, len(rest)))
    tail = np.flatnonzero(~np.isfinite(words[scv.n_folds * unit // 8:]))
    if len(tail):
        out.append(("behind the units", len(tail)))
    return out


class _NanWorkspaces:
    """``torch`` as cvmatrix_amd._stage.launch sees it, with one difference: a workspace starts with every byte 0xFF, a
    NaN in both element types.  Whatever a launch reads from its scratch without having written it is then a NaN."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        return torch.empty(*args, **kw).fill_(0xFF)


@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_a_stream_after_a_poisoned_one_has_the_bits_of_a_fresh_one(amd, dtype):
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    X, Y, w = shc.clean_problem(shc.K, shc.M, name)
    Xp, Yp = X.copy(), Y.copy()
    for f, c in ((0, 0), (0, 64), (3, 63), (3, 129)):
        Xp[folds[f][[0, -1]], c] = np.nan
        Yp[folds[f][1], c % shc.M] = np.nan
    rows = shc.chunk_rows("C", labels)
    clean_order = [rows[i] for i in (2, 4, 0, 3, 1)]          # the clean stream: another fold order
    fresh = _stream(amd, X, Y, w, labels, clean_order, hc.ON, dtype)
    assert not _nonfinite_places(fresh)
    want = _bits(fresh)
    assert all(bool(torch.isfinite(t.view(torch.float64 if dtype is np.float64 else torch.float32)).all()) for t in want)
    # poisoned, reset(), clean
    scv = _stream(amd, Xp, Yp, w, labels, rows, hc.ON, dtype)
    assert not _accumulator_is_finite(scv)
    poisoned_bits = _bits(scv)                                # (runs close, the finalize and the union kernels on NaN)
    assert not all(torch.equal(a, b) for a, b in zip(poisoned_bits, want))
    scv.reset()
    for r in clean_order:
        scv.partial_fit(X[r], Y[r], w[r], labels[r])
    assert not _nonfinite_places(scv)
    got = _bits(scv)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    # without reset(): a second object next to a poisoned one that is still alive
    other = _stream(amd, Xp, Yp, w, labels, rows, hc.ON, dtype)
    _bits(other)
    second = _stream(amd, X, Y, w, labels, clean_order, hc.ON, dtype)
    assert not _nonfinite_places(second) and not _accumulator_is_finite(other)
    got = _bits(second)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("chunking", ["B", "C"])
@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_the_accumulator_takes_nothing_the_chunk_did_not_write(amd, dtype, chunking, monkeypatch):
    """Every chunk's scratch full of NaN before its launches: a clean stream leaves a finite accumulator and the bits
    of a stream on other memory.  (The Gram launch writes neither the strictly lower 16 x 16 blocks of a diagonal tile
    -- nothing reads them -- nor the spare last word of a unit's statistics, and the accumulate kernel once added
    both: results were not affected, the accumulator held whatever the scratch had held.)"""
    import cvmatrix_amd._stage as stage
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    X, Y, w = shc.clean_problem(shc.K, shc.M, name)
    rows = shc.chunk_rows(chunking, labels)
    want = _bits(_stream(amd, X, Y, w, labels, rows, hc.ON, dtype))
    monkeypatch.setattr(stage, "torch", _NanWorkspaces())
    scv = _stream(amd, X, Y, w, labels, rows, hc.ON, dtype)
    assert not _nonfinite_places(scv)
    got = _bits(scv)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_a_chunk_without_rows_of_a_fold_leaves_its_unit_alone(amd, dtype):
    from cvmatrix_amd.streaming import _unit_layout
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    X, Y, w = shc.clean_problem(shc.K, shc.M, name)
    Xp = X.copy()
    Xp[folds[0][[0, 5, -1]], 64] = np.nan
    rows = shc.chunk_rows("C", labels)
    scv = _stream(amd, Xp, Y, w, labels, rows[:1], hc.ON, dtype)
    torch.cuda.synchronize()
    unit = _unit_layout(scv._cv._Kd, scv._cv._Md)[0]
    assert scv._acc.numel() >= shc.P * unit
    before = scv._acc.clone()
    assert bool(torch.isnan(before[:unit].view(torch.float64)).any()) and not before[unit:].any()
    scv.partial_fit(X[rows[1]], Y[rows[1]], w[rows[1]], labels[rows[1]])       # fold 1 alone: fold 0 has no row
    torch.cuda.synchronize()
    after = scv._acc
    assert torch.equal(after[:unit], before[:unit])                          # fold 0: the same bytes
    assert after[unit:2 * unit].any() and bool(torch.isfinite(after[unit:2 * unit].view(torch.float64)).all())
    assert not after[2 * unit:].any()                                        # folds 2, 3, 4: still nothing


# ---------------------------------------------------------------------------------------- cancellation ladder
def _ladder_params():
    return [pytest.param(dtype, off, run, id=f"{dtype.__name__}-{off:g}-{run}")
            for dtype in shc.DTYPES for off in hc.LADDER[dtype] for run in shc.ladder_runs()]


@pytest.mark.parametrize("dtype,off,run", _ladder_params())
def test_cancellation_ladder(amd, dtype, off, run):
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    X, Y, w = shc.ladder_problem(name, off, run)
    reference = shc.ladder_reference(name, off, run)
    flags = shc.run_settings(run)[0]
    for chunking in shc.LADDER_CHUNKINGS:
        scv = _stream(amd, X, Y, w, labels, shc.chunk_rows(chunking, labels), flags, dtype)
        shc.assert_ladder(_stream_items(scv, shc.ITEMS), reference, dtype, off, run, f"stream-{chunking}")
    got, cvm = _fitted_unions(amd, X, Y, w, folds, flags, dtype, shc.ITEMS)
    shc.assert_ladder(got, reference, dtype, off, run, "unions")
    assert cvm.fold_status() == 0


# ---------------------------------------------------------------------------------------- scale spread
@pytest.mark.parametrize("dtype,span,wspan", [pytest.param(*s, id=f"{s[0].__name__}-span{s[1]}") for s in hc.SPREADS])
def test_column_and_weight_scales_spread_over_decades(amd, dtype, span, wspan):
    name = np.dtype(dtype).name
    labels, folds = shc.design()
    reference = shc.spread_reference(name, span, wspan)
    X, Y, w = reference[:3]
    for flags in (hc.ON, hc.CENTRE_ONLY):
        for chunking in shc.SPREAD_CHUNKINGS:
            scv = _stream(amd, X, Y, w, labels, shc.chunk_rows(chunking, labels, w), flags, dtype)
            shc.assert_spread(_stream_items(scv, shc.ITEMS), reference, flags, dtype, f"stream-{chunking} span {span}")
        got, cvm = _fitted_unions(amd, X, Y, w, folds, flags, dtype, shc.ITEMS)
        shc.assert_spread(got, reference, flags, dtype, f"unions span {span}")
        assert cvm.fold_status() == 0


# ---------------------------------------------------------------------------------------- several row splits per chunk
@pytest.mark.parametrize("dtype", shc.DTYPES)
def test_ladder_rung_with_forced_row_splits(amd, dtype):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    name = np.dtype(dtype).name
    X, Y, w, labels, folds, cols, reference = shc.split_problem(name)
    try:
        assert lib.cvm_debug_force_splits(2, 3) == _lib.CVM_OK
        scv = amd.StreamingCVMatrix(5, *hc.ON, dtype=dtype)
        for r in (np.arange(0, 600), np.arange(600, 1200)):
            scv.partial_fit(X[r], Y[r], w[r], labels[r])
            assert scv._last_add[:2] == (2, 3), scv._last_add
        got = _stream_items(scv, shc.SPLIT_ITEMS)
    finally:
        lib.cvm_debug_force_splits(0, 0)
    shc.assert_ladder(got, reference, dtype, shc.SPLIT_RUNG[dtype], "weighted", "stream-splits", cols=cols, beyond=set())
