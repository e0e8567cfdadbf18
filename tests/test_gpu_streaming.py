"""GPU (-m gpu): streaming cross-validation (StreamingCVMatrix over cvm_stream_add / cvm_stream_close) against the
oracle fitted on all rows, the bit contracts of the accumulation, several row splits per chunk, float32, the
raises, and the consumers (ridge on streamed matrices, examples/streaming_cv_ridge.py against scikit-learn).

Tolerances.  float64: the project's gates, norm-wise 1e-10 for matrices and element-wise 1e-10 for statistics
(tests/test_streaming_host.py holds a NumPy model of the same sums within them on every case below).  float32:
the error against the float64 oracle on the float32-rounded inputs within fp32_gate.fp32_bound(yardstick), the
yardstick being the float32 oracle's own error -- the accumulator is float64 and rounds once per fold update."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import streaming_cases as sc
import unions_cases as uc
from conftest import assert_normwise, assert_stats, to_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


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


def none_pattern(stats):
    return tuple(s is None for s in stats)


def set_flags(scv, flags):
    scv.center_X, scv.center_Y, scv.scale_X, scv.scale_Y = flags


def stream(amd, X, Y, w, labels, rows, flags=(False,) * 4, dtype=np.float64, conv=lambda a: a, **kw):
    scv = amd.StreamingCVMatrix(uc.P, *flags, dtype=dtype, **kw)
    return sc.feed(scv, X, Y, w, labels, rows, conv)


def call(scv, method, *args):
    return getattr(scv, f"training_{method}")(*args)


def flat(res):
    mats, stats = res
    mats = list(mats) if isinstance(mats, tuple) else [mats]
    return mats + [s for s in stats if s is not None]


def same_bits(r1, r2):
    t1, t2 = flat(r1), flat(r2)
    assert len(t1) == len(t2)
    for a, b in zip(t1, t2):
        assert torch.equal(a, b)           # (NaN-free designs: a comparison of the bits up to the sign of zero)


# ---------------------------------------------------------------- 1. float64 parity
@pytest.mark.parametrize("pad", ["1", "0"], indirect=True)
@pytest.mark.parametrize("chunking", sc.CHUNKINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", uc.SHAPES)
def test_float64_parity(amd, K, M, weighted, chunking, pad):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    scv = stream(amd, X, Y, w, labels, sc.chunk_rows(chunking, labels))
    assert scv.N == uc.N and scv.fold_sizes.tolist() == list(uc.SIZES) and scv.n_chunks == {"A": 1, "C": 5}.get(chunking, 3)
    assert scv.accumulator_bytes > 0 and (scv.K, scv.M) == (K, M)
    for flags in uc.FLAGS:
        set_flags(scv, flags)
        for method in (uc.METHODS if M is not None else ("XTX",)):
            refs = sc.fold_reference(K, M, weighted, flags, method)
            what = f"K={K} M={M} w={weighted} {chunking} pad={pad} flags={flags} {method}"
            raised = [r for r in refs if isinstance(r, str)]
            if raised:
                with pytest.raises(ValueError) as e:
                    call(scv, method + "_batched")
                assert str(e.value) == raised[0], what
                continue
            gx, gy, gstats = uc.split_result(method, call(scv, method + "_batched"))
            for f in range(uc.P):
                rx, ry, rstats = uc.split_result(method, refs[f])
                if rx is not None:
                    assert_normwise(gx[f], rx, TOL, f"{what} fold {f} XTX")
                if ry is not None:
                    assert_normwise(gy[f], ry, TOL, f"{what} fold {f} XTY")
                assert_stats(tuple(None if s is None else s[f] for s in gstats), rstats, TOL, f"{what} fold {f}")
        # the statistics call
        srefs = sc.statistics_reference(K, M, weighted, flags)
        raised = [r for r in srefs if isinstance(r, str)]
        if raised:
            with pytest.raises(ValueError) as e:
                scv.training_statistics_batched()
            assert str(e.value) == raised[0]
        else:
            got = scv.training_statistics_batched()
            for f in range(uc.P):
                assert_stats(tuple(None if s is None else s[f] for s in got), srefs[f], TOL, f"{flags} statistics fold {f}")
        # the full-data attributes
        ref = sc.attribute_reference(K, M, weighted, flags)
        assert_normwise(scv.XTX, ref["XTX"], TOL, "XTX")
        if M is None:
            assert scv.XTY is None
        else:
            assert_normwise(scv.XTY, ref["XTY"], TOL, "XTY")
        for name in ("sum_X", "sum_sq_X", "sum_Y", "sum_sq_Y"):
            got = getattr(scv, name)
            assert (got is None) == (ref[name] is None), (flags, name)
            if got is not None:
                assert to_np(got).shape == ref[name].shape
                np.testing.assert_allclose(to_np(got), ref[name], rtol=TOL, atol=0, err_msg=name)
        for name in ("sum_w", "num_nonzero_w"):
            got = getattr(scv, name)
            assert (got is None) == (ref[name] is None), (flags, name)
            if got is not None:
                np.testing.assert_allclose(got, ref[name], rtol=TOL)


# ---------------------------------------------------------------- 2. unions of folds from the accumulated state
@pytest.mark.parametrize("pad", ["1", "0"], indirect=True)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", uc.SHAPES)
def test_every_union_under_chunking_B(amd, K, M, weighted, pad):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    scv = stream(amd, X, Y, w, labels, sc.chunk_rows("B", labels))
    for flags in uc.FLAGS:
        set_flags(scv, flags)
        for method in (uc.METHODS if M is not None else ("XTX",)):
            refs = uc.base_reference(K, M, weighted, flags, method)
            ok = [u for u, r in enumerate(refs) if not isinstance(r, str)]
            gx, gy, gstats = uc.split_result(method, call(scv, method + "_unions", [uc.UNIONS[u] for u in ok]))
            for i, u in enumerate(ok):
                rx, ry, rstats = uc.split_result(method, refs[u])
                what = f"K={K} M={M} w={weighted} flags={flags} {method} union {uc.UNIONS[u]}"
                if uc.weightless(weighted, uc.UNIONS[u]):
                    # (exactly zero matrices: the gate on the operands of the subtraction, as in test_gpu_unions.py)
                    sx, sy = uc.full_scale(K, M, weighted)
                    if rx is not None:
                        assert np.abs(to_np(gx[i]) - rx).max() <= TOL * sx, what + " XTX"
                    if ry is not None:
                        assert np.abs(to_np(gy[i]) - ry).max() <= TOL * sy, what + " XTY"
                    assert none_pattern(gstats) == none_pattern(rstats) == (True,) * 4
                    continue
                if rx is not None:
                    assert_normwise(gx[i], rx, TOL, what + " XTX")
                if ry is not None:
                    assert_normwise(gy[i], ry, TOL, what + " XTY")
                assert_stats(tuple(None if s is None else s[i] for s in gstats), rstats, TOL, what)
            assert len(ok) == len(refs) or weighted
            for u, r in enumerate(refs):                     # where the reference raises: the same message
                if isinstance(r, str):
                    with pytest.raises(ValueError) as e:
                        call(scv, method + "_unions", [uc.UNIONS[u]])
                    assert str(e.value) == r


# ---------------------------------------------------------------- 3. bit contracts (float64)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", [(7, 1), (64, 3), (130, 3)])
def test_one_chunk_has_the_bits_of_the_one_shot_sweep(amd, K, M, weighted):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    part = [np.array(f) for f in folds]                      # fold position = label
    scv = stream(amd, X, Y, w, labels, sc.chunk_rows("A", labels))
    for flags in ((True,) * 4, (False,) * 4, (True, False, True, False)):
        cvm = amd.CVMatrix(*flags, dtype=np.float64)
        cvm.fit(X, Y, w, folds=part)
        set_flags(scv, flags)
        same_bits(scv.training_XTX_XTY_batched(), cvm.training_XTX_XTY_batched(cvm.sweep_folds))
        assert torch.equal(scv.XTX, cvm.XTX) and torch.equal(scv.XTY, cvm.XTY)


def test_same_chunks_same_bits_and_snapshots(amd):
    X, Y, w, labels, folds = uc.base_design(130, 3, True)
    rows = [r for r in sc.chunk_rows("B", labels) if len(r)]
    flags = (True,) * 4
    first = stream(amd, X, Y, w, labels, rows, flags)
    r1 = first.training_XTX_XTY_batched()
    same_bits(stream(amd, X, Y, w, labels, rows, flags).training_XTX_XTY_batched(), r1)
    # a snapshot after two chunks, then the third chunk: a fresh three-chunk stream
    scv = stream(amd, X, Y, w, labels, rows[:2], flags)
    early = scv.training_XTX_XTY_batched()
    kept = [t.clone() for t in flat(early)]
    early_unions = scv.training_XTX_XTY_unions([[0, 1], [2]])
    same_bits(scv.training_XTX_XTY_batched(), early)         # (close does not disturb the accumulator)
    sc.feed(scv, X, Y, w, labels, rows[2:])
    same_bits(scv.training_XTX_XTY_batched(), r1)
    same_bits(scv.training_XTX_XTY_unions([[0, 1], [2]]), first.training_XTX_XTY_unions([[0, 1], [2]]))
    for a, b in zip(flat(early), kept):                      # what the early snapshot handed out stays as it was
        assert torch.equal(a, b)
    assert not torch.equal(flat(early_unions)[0], flat(first.training_XTX_XTY_unions([[0, 1], [2]]))[0])
    # device tensors as chunks: the same bits as host arrays
    dev = stream(amd, X, Y, w, labels, rows, flags, conv=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    same_bits(dev.training_XTX_XTY_batched(), r1)


# ---------------------------------------------------------------- 4. several row splits per chunk
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_chunks_with_forced_row_splits(amd, dtype):
    from cvmatrix_amd import _lib
    from cvmatrix_amd.fp32_gate import fp32_bound
    lib = _lib.load()
    name = np.dtype(dtype).name
    X, Y, w, labels, folds = uc.split_design(name)
    try:
        assert lib.cvm_debug_force_splits(2, 3) == _lib.CVM_OK
        scv = amd.StreamingCVMatrix(5, dtype=dtype)
        for r in (np.arange(0, 600), np.arange(600, 1200)):
            scv.partial_fit(X[r], Y[r], w[r], labels[r])
            # (the plan token of the chunk's own Gram launch, as the library reports it)
            assert scv._last_add[:2] == (2, 3), scv._last_add
        for flags in ((True,) * 4, (False,) * 4):
            set_flags(scv, flags)
            ref64, refdt = sc.split_reference(name, flags)
            (gx, gy), gstats = scv.training_XTX_XTY_batched()
            assert gx.dtype == (torch.float64 if dtype is np.float64 else torch.float32)
            for f in range(5):
                for got, i, what in ((gx[f], 0, "XTX"), (gy[f], 1, "XTY")):
                    if dtype is np.float64:
                        assert_normwise(got, ref64[f][0][i], TOL, f"{flags} fold {f} {what}")
                    else:
                        err, yard = sc.fp32_errors(to_np(got), ref64[f][0][i], refdt[f][0][i])
                        assert err <= fp32_bound(yard), (flags, f, what, err, yard)
                if dtype is np.float64:
                    assert_stats(tuple(None if s is None else s[f] for s in gstats), ref64[f][1], TOL, f"{flags} fold {f}")
                else:
                    assert none_pattern(gstats) == none_pattern(ref64[f][1])
    finally:
        lib.cvm_debug_force_splits(0, 0)


# ---------------------------------------------------------------- 5. float32
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", [(64, 3), (130, 3)])
def test_float32_within_the_reference_float32_error(amd, K, M, weighted):
    from cvmatrix_amd.fp32_gate import fp32_bound
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    c = lambda a: a.astype(np.float32)      # noqa: E731
    scv = stream(amd, X, Y, w, labels, sc.chunk_rows("B", labels), dtype=np.float32, conv=c)
    for flags in uc.FLAGS:
        set_flags(scv, flags)
        ref64, ref32 = sc.fold_reference32(K, M, weighted, flags)
        assert not any(isinstance(r, str) for r in ref64 + ref32)
        (gx, gy), gstats = scv.training_XTX_XTY_batched()
        assert gx.dtype == torch.float32 and none_pattern(gstats) == none_pattern(ref64[0][1])
        for f in range(uc.P):
            for name, got, i in (("XTX", gx[f], 0), ("XTY", gy[f], 1)):
                err, yard = sc.fp32_errors(to_np(got), ref64[f][0][i], ref32[f][0][i])
                assert err <= fp32_bound(yard), (K, weighted, flags, f, name, err, yard)


# ---------------------------------------------------------------- 6. raises
def test_negative_weights(amd):
    from cvmatrix_amd.cvmatrix import MSG_NEG_W
    X, Y, w, labels, folds = uc.base_design(64, 3, True)
    rows = [r for r in sc.chunk_rows("B", labels) if len(r)]
    bad = w[rows[1]].copy()
    bad[0] = -1.0
    # host chunk: raised by partial_fit before the upload; the results equal the stream without that chunk
    scv = stream(amd, X, Y, w, labels, rows[:1], (True,) * 4)
    with pytest.raises(ValueError) as e:
        scv.partial_fit(X[rows[1]], Y[rows[1]], bad, labels[rows[1]])
    assert str(e.value) == MSG_NEG_W and scv.n_chunks == 1
    sc.feed(scv, X, Y, w, labels, rows[2:])
    without = stream(amd, X, Y, w, labels, [rows[0], rows[2]], (True,) * 4)
    same_bits(scv.training_XTX_XTY_batched(), without.training_XTX_XTY_batched())
    # device chunk: raised at hand-out, and again, until reset()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    scv = stream(amd, X, Y, w, labels, rows[:1], (True,) * 4)
    scv.partial_fit(cu(X[rows[1]]), cu(Y[rows[1]]), cu(bad), labels[rows[1]])
    sc.feed(scv, X, Y, w, labels, rows[2:])
    for hand_out in (scv.training_XTX_XTY_batched, scv.training_statistics_batched, lambda: scv.XTX,
                     lambda: scv.training_XTX_unions([[0, 1]]), scv.training_XTX_batched):
        with pytest.raises(ValueError) as e:
            hand_out()
        assert str(e.value) == MSG_NEG_W
    scv.reset()
    assert scv.N == 0 and scv.n_chunks == 0
    sc.feed(scv, X, Y, w, labels, rows)
    same_bits(scv.training_XTX_XTY_batched(), stream(amd, X, Y, w, labels, rows, (True,) * 4).training_XTX_XTY_batched())


def test_data_dependent_raises(amd):
    from cvmatrix_amd.cvmatrix import MSG_NZ_DDOF, MSG_NZ_ZERO
    X, Y, _, labels, folds = uc.base_design(64, 3, False)
    rows = sc.chunk_rows("B", labels)
    w = np.where(labels == 0, 1.0, 0.0)                      # weights zero outside fold 0
    scv = stream(amd, X, Y, w, labels, rows, (True, False, False, False))
    for hand_out in (scv.training_XTX_XTY_batched, scv.training_XTX_batched, scv.training_statistics_batched,
                     lambda: scv.training_XTX_unions([[0]])):
        with pytest.raises(ValueError) as e:
            hand_out()
        assert str(e.value) == MSG_NZ_ZERO
    scv.training_XTX_unions([[1], [2, 3]])                   # (their training sets keep fold 0)
    set_flags(scv, (False,) * 4)                             # without centring or scaling the counts are not looked at
    scv.training_XTX_XTY_batched()
    scv.training_XTX_XTY_unions([[0]])
    # ddof: unweighted, the training set of fold 0 holds 203 - 67 = 136 rows
    for ddof, raises in ((136, True), (135, False)):
        scv = amd.StreamingCVMatrix(uc.P, False, False, True, False, ddof=ddof)
        sc.feed(scv, X, Y, None, labels, rows)
        if raises:
            with pytest.raises(ValueError) as e:
                scv.training_XTX_batched()
            assert str(e.value) == MSG_NZ_DDOF
            scv.scale_X, scv.center_X = False, True          # centring alone needs no more than one non-zero weight
            scv.training_XTX_batched()
        else:
            scv.training_XTX_batched()


def test_refused_chunks_leave_the_accumulator_alone(amd):
    X, Y, w, labels, folds = uc.base_design(64, 3, True)
    rows = [r for r in sc.chunk_rows("B", labels) if len(r)]
    scv = stream(amd, X, Y, w, labels, rows[:2])
    before, state = scv._acc.clone(), scv._state.copy()
    r = rows[2]
    bad_lab = labels[r].copy()
    bad_lab[3] = uc.P
    for args in ((X[r][:, :63], Y[r], w[r], labels[r]), (X[r], None, w[r], labels[r]), (X[r], Y[r][:, :2], w[r], labels[r]),
                 (X[r], Y[r], None, labels[r]), (X[r], Y[r], w[r], bad_lab), (X[r], Y[r], w[r], labels[r][:-1])):
        with pytest.raises(ValueError):
            scv.partial_fit(*args)
    torch.cuda.synchronize()
    assert torch.equal(scv._acc, before) and np.array_equal(scv._state, state) and scv.n_chunks == 2
    with pytest.raises(ValueError):
        scv.training_XTX_unions([[0, 0]])
    noY = amd.StreamingCVMatrix(uc.P)
    sc.feed(noY, X, None, None, labels, rows)
    with pytest.raises(ValueError):
        noY.training_XTY_batched()
    with pytest.raises(ValueError):
        noY.training_XTX_XTY_unions([[0]])


def test_c_entry_points_refuse_before_the_device_is_touched(amd):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    P, K, M, n = 3, 8, 2, 12
    dev = torch.device("cuda:0")
    vp = ctypes.c_void_p
    acc_bytes = lib.cvm_stream_workspace_bytes(_lib.STREAM_ACCUMULATOR, P, 0, K, M, _lib.CVM_F64)
    ws_bytes = lib.cvm_stream_workspace_bytes(_lib.STREAM_SCRATCH, P, n, K, M, _lib.CVM_F64)
    assert acc_bytes > 0 and ws_bytes > 0 and lib.cvm_stream_workspace_bytes(_lib.STREAM_CLOSE, P, 0, K, M, _lib.CVM_F64) == 0
    assert lib.cvm_stream_workspace_bytes(_lib.STREAM_CLOSE, P, 0, K, M, _lib.CVM_F32) > 0
    assert lib.cvm_stream_workspace_bytes(7, P, 0, K, M, _lib.CVM_F64) == 0
    acc = torch.empty(acc_bytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    state = np.zeros(_lib.STREAM_STATE_LEN, dtype=np.int64)
    rng = np.random.default_rng(3)
    X, Y = torch.from_numpy(rng.standard_normal((n, K))).to(dev), torch.from_numpy(rng.standard_normal((n, M))).to(dev)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    good = np.array([0, 5, 5, 12], dtype=np.int64)
    offs = torch.from_numpy(good).to(dev)

    def add(host_offsets=good, n_folds=P, n_rows=n, k=K, m=M, dtype=_lib.CVM_F64, acc_b=acc_bytes, ws_b=ws_bytes, st=state, y=Y):
        return lib.cvm_stream_add(X.data_ptr(), _lib.ptr(y), 0, idx.data_ptr(), offs.data_ptr(), host_offsets.ctypes.data,
                                  n_folds, n_rows, k, m, dtype, acc.data_ptr(), acc_b, st.ctypes.data, ws.data_ptr(), ws_b, 0, 0)
    assert add() == _lib.CVM_EINVAL                           # no header yet
    assert lib.cvm_stream_reset(acc.data_ptr(), acc_bytes - 256, P, K, M, _lib.CVM_F64, state.ctypes.data, 0) == _lib.CVM_EWORKSPACE
    assert lib.cvm_stream_reset(acc.data_ptr(), acc_bytes, 0, K, M, _lib.CVM_F64, state.ctypes.data, 0) == _lib.CVM_EINVAL
    assert lib.cvm_stream_reset(acc.data_ptr(), acc_bytes, P, K, M, _lib.CVM_F64, state.ctypes.data, 0) == _lib.CVM_OK
    torch.cuda.synchronize()
    assert not acc.any()
    assert add() == _lib.CVM_OK                               # (a good chunk first: something to leave unchanged)
    torch.cuda.synchronize()
    before, header = acc.clone(), state.copy()
    assert before.any() and header[5] == 1 and header[6] == n
    einval = (dict(n_rows=-1), dict(host_offsets=np.array([0, 7, 5, 12], dtype=np.int64)),
              dict(host_offsets=np.array([0, 5, 5, 11], dtype=np.int64)), dict(host_offsets=np.array([-1, 5, 5, 11], dtype=np.int64)),
              dict(k=K + 1), dict(m=M + 1), dict(m=0, y=None), dict(dtype=_lib.CVM_F32), dict(dtype=5), dict(n_folds=P + 1),
              dict(n_folds=0), dict(st=np.zeros(_lib.STREAM_STATE_LEN, dtype=np.int64)), dict(y=None))
    for kw in einval:
        assert add(**kw) == _lib.CVM_EINVAL, kw
    for kw in (dict(acc_b=acc_bytes - 256), dict(ws_b=1024), dict(ws_b=0)):
        assert add(**kw) == _lib.CVM_EWORKSPACE, kw
    assert add(host_offsets=np.zeros(P + 1, dtype=np.int64), n_rows=0) == _lib.CVM_OK      # an empty chunk: no launch
    G = torch.empty((K, K), dtype=torch.float64, device=dev)
    H = torch.empty((K, M), dtype=torch.float64, device=dev)
    gs = torch.empty(lib.cvm_gstats_len(K, M), dtype=torch.float64, device=dev)
    units, nbytes, token = vp(0), ctypes.c_size_t(0), ctypes.c_int64(0)

    def close(n_folds=P, k=K, dtype=_lib.CVM_F64, acc_b=acc_bytes, g=G, ws_p=0, ws_b=0):
        return lib.cvm_stream_close(acc.data_ptr(), acc_b, state.ctypes.data, n_folds, k, M, dtype, _lib.ptr(g), H.data_ptr(),
                                    gs.data_ptr(), 0, ws_p, ws_b, 0, ctypes.byref(units), ctypes.byref(nbytes), ctypes.byref(token))
    for kw in (dict(n_folds=P + 1), dict(k=K + 2), dict(dtype=_lib.CVM_F32, ws_p=ws.data_ptr(), ws_b=ws_bytes), dict(g=None)):
        assert close(**kw) == _lib.CVM_EINVAL, kw
    assert close(acc_b=acc_bytes - 256) == _lib.CVM_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(acc, before) and np.array_equal(state, header)
    assert close() == _lib.CVM_OK
    torch.cuda.synchronize()
    assert units.value == acc.data_ptr() and nbytes.value == acc_bytes and token.value == (1 | (1 << 20))
    Xh = X.cpu().numpy()
    assert_normwise(G, Xh.T @ Xh, TOL, "G")
    assert_normwise(H, Xh.T @ Y.cpu().numpy(), TOL, "H")
    assert torch.equal(acc, before)                           # close does not write the accumulator
    # float32: the close workspace too small
    state32 = np.zeros(_lib.STREAM_STATE_LEN, dtype=np.int64)
    assert lib.cvm_stream_reset(acc.data_ptr(), acc_bytes, P, K, M, _lib.CVM_F32, state32.ctypes.data, 0) == _lib.CVM_OK
    G32, H32 = G.float(), H.float()
    rc = lib.cvm_stream_close(acc.data_ptr(), acc_bytes, state32.ctypes.data, P, K, M, _lib.CVM_F32, G32.data_ptr(), H32.data_ptr(),
                              gs.data_ptr(), 0, ws.data_ptr(), 256, 0, ctypes.byref(units), ctypes.byref(nbytes), ctypes.byref(token))
    assert rc == _lib.CVM_EWORKSPACE
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. consumer and example
def test_ridge_on_streamed_matrices(amd):
    from cvmatrix_amd.ridge import ridge_fit_batched
    X, Y, w, labels, folds = uc.base_design(64, 3, True)
    flags = (True, True, False, False)
    scv = stream(amd, X, Y, w, labels, sc.chunk_rows("B", labels), flags)
    (XTX, XTY), stats = scv.training_XTX_XTY_batched()
    cvm = amd.CVMatrix(*flags, dtype=np.float64)
    cvm.fit(X, Y, w)
    (RXX, RXY), rstats = cvm.training_XTX_XTY_batched([np.array(f) for f in folds])
    lam = np.array([0.01, 1.0, 50.0])
    B, RB = ridge_fit_batched(XTX, XTY, lam).B, ridge_fit_batched(RXX, RXY, lam).B
    assert B.shape == RB.shape == (uc.P, 3, 64, 3)
    for f in range(uc.P):
        for l in range(3):
            assert_normwise(B[f, l], to_np(RB[f, l]), TOL, f"fold {f} lambda {l}")


@pytest.mark.parametrize("weighted", [False, True])
def test_streaming_example_against_sklearn_refits(amd, weighted):
    import sklearn.linear_model as lm
    spec = importlib.util.spec_from_file_location("streaming_cv_ridge", os.path.join(ROOT, "examples", "streaming_cv_ridge.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rng = np.random.default_rng(11)
    N, K, M, P = 300, 20, 2, 5
    X = rng.standard_normal((N, K))
    Y = X @ rng.standard_normal((K, M)) + 0.5 * rng.standard_normal((N, M)) + 2.0
    w = rng.random(N) + 0.2 if weighted else None
    labels = np.arange(N) % P
    lam = np.array([0.01, 1.0, 50.0])
    bounds = [0, 90, 200, 300]                               # three chunks, each with rows of every fold

    def chunks():
        for a, b in zip(bounds[:-1], bounds[1:]):
            yield X[a:b], Y[a:b], None if w is None else w[a:b], labels[a:b]
    got = ex.streaming_cv_rmse(chunks, P, lam)
    sse, wsum = np.zeros((lam.size, M)), 0.0
    for f in range(P):
        val, tr = labels == f, labels != f
        wv = np.ones(int(val.sum())) if w is None else w[val]
        wsum += wv.sum()
        for l, lv in enumerate(lam):
            pred = lm.Ridge(alpha=lv, fit_intercept=True).fit(X[tr], Y[tr], None if w is None else w[tr]).predict(X[val])
            sse[l] += wv @ (pred.reshape(-1, M) - Y[val]) ** 2
    np.testing.assert_allclose(got, np.sqrt(sse / wsum), rtol=1e-9)
