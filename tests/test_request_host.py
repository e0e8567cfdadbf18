"""CPU: the Python host layer -- the fold request (which statistics a call returns, the C ABI flag word, the
shape of the return value) against the oracle and the library's constants, and the front door of the fitters'
refusal of host data before any device is touched."""

import itertools

import numpy as np
import pytest
import torch

from cvmatrix_amd import _lib, _stage
from cvmatrix_amd._request import FoldRequest, fold_request, stat_addresses
from oracle.cvmatrix_oracle import OracleCVMatrix

# every (rXTX, rXTY, cX, cY, sX, sY) of the 64 with at least one matrix returned
REQUESTS = [c for c in itertools.product((False, True), repeat=6) if c[0] or c[1]]


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(3)
    return rng.random((6, 3)), rng.random((6, 2))


@pytest.mark.parametrize("combo", REQUESTS, ids=lambda c: "".join("01"[b] for b in c))
def test_want_is_the_oracles_none_pattern_and_flags_are_the_abi_bits(problem, combo):
    rXTX, rXTY, cX, cY, sX, sY = combo
    X, Y = problem
    o = OracleCVMatrix(cX, cY, sX, sY, ddof=0)
    o.fit(X, Y)
    call = o.training_XTX_XTY if rXTX and rXTY else (o.training_XTX if rXTX else o.training_XTY)
    _, stats = call(np.array([0, 1]))
    req = fold_request(*combo)
    assert req.want == tuple(s is not None for s in stats)
    assert req.need_stats == any(req.want) and req.need_std == (req.want[1] or req.want[3])
    bits = (_lib.RET_XTX, _lib.RET_XTY, _lib.CENTER_X, _lib.CENTER_Y, _lib.SCALE_X, _lib.SCALE_Y)
    assert req.flags == sum(b for b, on in zip(bits, combo) if on) and not req.flags & _lib.IDX_HOST
    assert fold_request(*combo) is req                  # one shared record per combination
    assert fold_request(*(int(b) for b in combo)) is req and fold_request(*(np.bool_(b) for b in combo)).want == req.want


@pytest.mark.parametrize("combo", REQUESTS, ids=lambda c: "".join("01"[b] for b in c))
def test_pack_nests_like_the_reference_and_drops_what_is_not_wanted(combo):
    req = fold_request(*combo)
    xtx, xty, st = object(), object(), [object() for _ in range(4)]
    mats, stats = req.pack(xtx, xty, *st)
    if combo[0] and combo[1]:
        assert type(mats) is tuple and mats[0] is xtx and mats[1] is xty
    else:
        assert mats is (xtx if combo[0] else xty)
    assert type(stats) is tuple and len(stats) == 4
    for got, given, w in zip(stats, st, req.want):
        assert got is (given if w else None)
    # converters see exactly what is kept; ``at`` takes one fold of stacked results and touches nothing else
    tag = tuple((lambda t, k=k: (k, t)) for k in ("XX", "XY", "X", "Y"))
    stacked = [None if not keep else [10 * i, 10 * i + 1] for i, keep in enumerate((combo[0], combo[1], *req.want))]
    mats, stats = req.pack(*stacked, tag, at=1)
    flat = (mats if combo[0] and combo[1] else (mats,)) + stats
    want = [(k, 10 * i + 1) for i, (k, keep) in enumerate(zip(("XX", "XY", "X", "X", "Y", "Y"), (combo[0], combo[1], *req.want)))
            if keep]
    assert [f for f in flat if f is not None] == want


def test_pack_one_carves_the_wanted_blocks_of_a_flat_statistics_vector():
    K, M = 3, 2
    stat = torch.arange(2 * K + 2 * M, dtype=torch.float64)
    (xtx, xty), (muX, sdX, muY, sdY) = fold_request(True, True, True, True, True, True).pack_one("G", "H", stat, K, M)
    assert (xtx, xty) == ("G", "H")
    assert muX.tolist() == [[0, 1, 2]] and sdX.tolist() == [[3, 4, 5]] and muY.tolist() == [[6, 7]] and sdY.tolist() == [[8, 9]]
    assert muX.data_ptr() == stat.data_ptr()            # views, no copies
    mats, stats = FoldRequest(True, False, False, False, True, False).pack_one("G", None, stat, K, M)
    assert mats == "G" and stats[0] is None and stats[1].tolist() == [[3, 4, 5]] and stats[2:] == (None, None)
    assert stat_addresses(1000, 8, K, M) == (1000, 1024, 1048, 1064) and stat_addresses(1000, 4, K, 0) == (1000, 1012, 0, 0)


@pytest.mark.parametrize("y_optional", [False, True])
def test_training_pair_refuses_host_data_before_the_device(y_optional):
    G, H = torch.eye(3, dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64)
    for XTX, XTY in ((G, H), (G.numpy(), H.numpy()), (G, H.numpy()), (G, None), ([[1.0]], [[1.0]])):
        with pytest.raises(TypeError, match="fitter takes device tensors"):
            _stage.training_pair("fitter", XTX, XTY, y_optional=y_optional)


def test_stat_tensor_refuses_host_data_before_the_device():
    for t in (torch.ones((2, 3), dtype=torch.float64), np.ones((2, 3)), [1.0, 2.0]):
        with pytest.raises(TypeError):
            _stage.stat_tensor("mean of X", t, 2, 3, torch.float64, torch.device("cuda", 0))
    assert _stage.stat_tensor("mean of X", None, 2, 3, torch.float64, torch.device("cuda", 0)) is None
    with pytest.raises(ValueError):
        _stage.stat_tensors((None, None, None), 2, 3, 1, torch.float64, torch.device("cuda", 0))


def test_dtype_code():
    assert _stage.dtype_code(torch.float64) == _lib.CVM_F64 and _stage.dtype_code(torch.float32) == _lib.CVM_F32
