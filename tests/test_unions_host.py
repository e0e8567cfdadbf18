"""CPU: the host half of the unions of folds -- the lists nested cross-validation needs (against itertools),
the checks of a caller's list, workspace sizing and every refusal of cvm_sweep_unions through the C ABI
(decided before the device is touched: none is there), and the golden file against the oracle."""

import itertools

import numpy as np
import pytest

import unions_cases as uc
from conftest import assert_normwise, assert_stats, golden_stats, load_npz
from cvmatrix_amd import _lib
from cvmatrix_amd import unions as un
from oracle.cvmatrix_oracle import OracleCVMatrix


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("P", [0, 1, 2, 3, 5, 10, 20])
def test_fold_pairs_and_nested_units_against_itertools(P):
    pairs = un.fold_pairs(P)
    assert pairs.dtype == np.int64 and pairs.shape == (P * (P - 1) // 2, 2)
    assert [tuple(r) for r in pairs] == list(itertools.combinations(range(P), 2))
    outer, pair, inner = un.nested_units(P)
    assert outer.dtype == pair.dtype == inner.dtype == np.int64
    assert list(zip(outer, inner)) == list(itertools.permutations(range(P), 2))
    lookup = {frozenset(c): i for i, c in enumerate(itertools.combinations(range(P), 2))}
    assert list(pair) == [lookup[frozenset((f, g))] for f, g in itertools.permutations(range(P), 2)]
    for f, q, g in zip(outer, pair, inner):
        assert set(pairs[q]) == {f, g}


def test_prepare_unions_checks_and_sorts():
    ub = un.prepare_unions([[3, 1], (0,), np.array([4, 2, 0])], 5)
    assert ub.n_unions == 3 and ub.folds.dtype == ub.offsets.dtype == np.int64
    assert ub.folds.tolist() == [1, 3, 0, 0, 2, 4] and ub.offsets.tolist() == [0, 2, 3, 6]
    assert un.prepare_unions(un.fold_pairs(4), 4).offsets.tolist() == list(range(0, 13, 2))
    assert un.prepare_unions([], 5).n_unions == 0
    assert un.prepare_unions(ub, 5) is ub
    for bad in ([[0, 0]], [[1, 2, 1]], [[5]], [[-1]], [[]], [[0], []], np.zeros((2, 0), dtype=int), [[0.5]],
                np.arange(3)):
        with pytest.raises(ValueError):
            un.prepare_unions(bad, 5)
    with pytest.raises(ValueError):
        un.prepare_unions(ub, 6)


def test_refused_where_the_globals_are_exchanged():
    """A model whose full-data matrices are exchanged between processes (ShardedCVMatrix with more than one
    rank) has no sweep of the whole data set on one device: the methods say so, before anything else."""
    from cvmatrix_amd import CVMatrix

    class Exchanging(CVMatrix):
        def _exchanges_globals(self):
            return True

    m = Exchanging()
    for name in ("training_XTX_unions", "training_XTY_unions", "training_XTX_XTY_unions"):
        with pytest.raises(NotImplementedError):
            getattr(m, name)([np.arange(3)], [[0]])
    with pytest.raises(RuntimeError):
        CVMatrix().training_XTX_unions([np.arange(3)], [[0]])


def test_workspace_bytes_is_monotone(lib):
    ws = lib.cvm_sweep_unions_workspace_bytes
    assert ws(1, 7, 1) >= (2 * 7 + 2 * 1 + 4) * 8
    for K, M in ((1, 0), (7, 1), (130, 3), (512, 16), (4096, 64)):
        last = 0
        for n in (0, 1, 2, 3, 45, 190, 1000, 10 ** 6):
            v = ws(n, K, M)
            assert v >= max(n, 1) * (2 * K + 2 * M + 4) * 8 and v >= last
            last = v
        assert ws(45, K + 1, M) >= ws(45, K, M) and ws(45, K, M + 1) >= ws(45, K, M)
    assert ws(-1, 8, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 8, -1) == 0


def _call(lib, **kw):
    """cvm_sweep_unions with made-up non-null addresses (nothing is dereferenced on the device: every case is
    refused, or launches nothing, before the device is touched); keyword arguments replace the defaults."""
    K, M = kw.pop("K", 8), kw.pop("M", 2)
    hoffs = np.asarray(kw.pop("hoffs", [0, 2, 3]), dtype=np.int64)
    a = dict(fold_offsets=64, n_total=5, union_folds=64, union_offsets=64, host=hoffs.ctypes.data, n_unions=len(hoffs) - 1,
             K=K, M=M, dtype=_lib.CVM_F64, flags=_lib.RET_XTX | _lib.RET_XTY, ddof=1.0, res=1e-14, weighted=0,
             G=64, H=64, gstats=64, oXX=64, oXY=64, muX=64, sdX=64, muY=64, sdY=64, ofold=0,
             sws=64, sws_bytes=1 << 40, splits=1 | (1 << 20), ws=64, ws_bytes=1 << 30, stream=0)
    a.update(kw)
    return lib.cvm_sweep_unions(*a.values())


def test_every_refusal_is_decided_without_a_device(lib):
    EI, EW = _lib.CVM_EINVAL, _lib.CVM_EWORKSPACE
    # (the accepted call that launches nothing: no union)
    assert _call(lib, hoffs=[0]) == _lib.CVM_OK
    assert _call(lib, hoffs=[7]) == _lib.CVM_OK
    # bad tokens
    for tok in (0, -1, 1, 1 << 20, 5 << 41 | 1 | 1 << 20):
        assert _call(lib, splits=tok) == EI, tok
    assert b"token" in lib.cvm_last_error()
    # null pointers that are needed
    for name in ("fold_offsets", "union_folds", "union_offsets", "host", "G", "gstats", "sws", "ws", "oXX", "oXY", "H"):
        assert _call(lib, **{name: 0}) == EI, name
    # shapes, dtype
    assert _call(lib, n_unions=-1) == EI
    assert _call(lib, n_total=0) == EI and _call(lib, K=0) == EI and _call(lib, M=-1) == EI
    assert _call(lib, dtype=7) == EI
    assert _call(lib, M=0) == EI                                     # CVM_RET_XTY without Y
    # union offsets: negative, decreasing, a union of no fold, more folds than there are
    for hoffs in ([-1, 1], [0, 2, 1], [0, 2, 2], [0, 0], [3, 3, 4], [0, 6]):
        assert _call(lib, hoffs=hoffs) == EI, hoffs
    # short workspaces
    need = lib.cvm_sweep_unions_workspace_bytes(2, 8, 2)
    assert _call(lib, ws_bytes=need - 1) == EW
    assert b"cvm_sweep_unions_workspace_bytes" in lib.cvm_last_error()
    assert _call(lib, sws_bytes=1024) == EW
    assert _call(lib, sws_bytes=0) == EW


@pytest.mark.parametrize("name,flags", [("1111", (True,) * 4), ("0000", (False,) * 4)])
def test_golden_unions_against_the_oracle(name, flags):
    """tests/golden/g9_unions.npz (the reference on the concatenated validation indices) against the oracle."""
    z = load_npz("g9_unions.npz")
    folds, unions = uc.golden_folds(z), uc.golden_unions(z)
    assert len(unions) == 11 and sorted(len(u) for u in unions) == [2] * 10 + [3]
    assert sorted(np.concatenate(folds).tolist()) == list(range(60))
    o = OracleCVMatrix(*flags)
    o.fit(z["X"], z["Y"], z["w"])
    for u, S in enumerate(unions):
        (xtx, xty), stats = o.training_XTX_XTY(uc.union_indices(folds, S))
        assert_normwise(xtx, z[f"{name}/{u}/XTX"], 1e-10, f"{name} union {u} XTX")
        assert_normwise(xty, z[f"{name}/{u}/XTY"], 1e-10, f"{name} union {u} XTY")
        assert_stats(stats, golden_stats(z, f"{name}/{u}"), 1e-10, f"{name} union {u}")
