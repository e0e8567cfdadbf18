"""CPU: a NumPy model of the streaming algebra, held against the gates of tests/test_gpu_streaming.py for every
case of its grid -- the check that the gates are attainable by the arithmetic the kernels are asked to do --
and the argument rules of StreamingCVMatrix that need no device.

The model: per chunk and fold the raw update (X_f' W X_f, X_f' W Y_f, column sums, sums of squares, sw, nz),
added to a float64 accumulator; float32: the chunk updates formed in float32, accumulated in float64, rounded
once; G = sum_f U_f in fold order; then the oracle's finish (cvmatrix_oracle.OracleCVMatrix._stats / _kernel)
in float64, rounded to the result type once."""

import numpy as np
import pytest

import streaming_cases as sc
import unions_cases as uc
from conftest import assert_normwise, assert_stats
from oracle.cvmatrix_oracle import MSG_NZ_DDOF, MSG_NZ_ZERO

TOL = 1e-10


# ---------------------------------------------------------------- the model
def accumulate(X, Y, w, labels, rows, P, dt):
    """Per fold: dict of the accumulated raw update (float64), chunk updates formed in ``dt``."""
    K = X.shape[1]
    M = 0 if Y is None else Y.shape[1]
    acc = [dict(U=np.zeros((K, K)), V=np.zeros((K, M)), s=np.zeros(K), q=np.zeros(K), sy=np.zeros(M), qy=np.zeros(M),
                sw=0.0, nz=0.0, n=0) for _ in range(P)]
    for r in rows:
        for f in range(P):
            rf = r[labels[r] == f]
            if rf.size == 0:
                continue                                     # (a fold without rows in the chunk is skipped)
            Xc = X[rf].astype(dt)
            wc = None if w is None else w[rf].astype(dt).reshape(-1, 1)
            WX = Xc if wc is None else Xc * wc
            a = acc[f]
            a["U"] += (WX.T @ Xc).astype(np.float64)
            # (the statistics of a unit are float64 in both dtypes)
            WX64, X64 = WX.astype(np.float64), Xc.astype(np.float64)
            a["s"] += WX64.sum(axis=0)
            a["q"] += (WX64 * X64).sum(axis=0)
            if Y is not None:
                Yc = Y[rf].astype(dt)
                a["V"] += (WX.T @ Yc).astype(np.float64)
                WY64 = Yc.astype(np.float64) if wc is None else Yc.astype(np.float64) * wc.astype(np.float64)
                a["sy"] += WY64.sum(axis=0)
                a["qy"] += (WY64 * Yc.astype(np.float64)).sum(axis=0)
            a["sw"] += float(rf.size) if wc is None else float(wc.astype(np.float64).sum())
            a["nz"] += float(rf.size) if wc is None else float(np.count_nonzero(wc))
            a["n"] += rf.size
    for a in acc:                                            # one rounding per fold update
        a["U"], a["V"] = a["U"].astype(dt).astype(np.float64), a["V"].astype(dt).astype(np.float64)
    return acc


def close(acc, dt):
    """G, H, column sums and totals: the fold-ordered sums of the units."""
    tot = {k: sum((a[k] for a in acc[1:]), acc[0][k] * 1.0) for k in ("U", "V", "s", "q", "sy", "qy", "sw", "nz")}
    tot["U"], tot["V"] = tot["U"].astype(dt).astype(np.float64), tot["V"].astype(dt).astype(np.float64)
    return tot


def finish(tot, upd, flags, method, ddof, dt, weighted, hasY):
    """The oracle's finish for the validation update ``upd`` (a fold's, or the sum of a union's folds')."""
    cX, cY, sX, sY = flags
    rXTX, rXTY = method in ("XTX", "XTX_XTY"), method in ("XTY", "XTX_XTY")
    mean_X, std_X = cX or (rXTY and cY), sX
    mean_Y, std_Y = rXTY and (cX or cY), rXTY and sY
    resolution = np.finfo(dt).resolution * 10
    muX = sdX = muY = sdY = None
    sw_t = None
    if mean_X or std_X or mean_Y or std_Y:
        sw_t, nz_t = tot["sw"] - upd["sw"], tot["nz"] - upd["nz"]
        if weighted and nz_t == 0:
            raise ValueError(MSG_NZ_ZERO)
        if std_X or std_Y:
            if nz_t <= ddof:
                raise ValueError(MSG_NZ_DDOF)
            divisor = (nz_t - ddof) * sw_t / nz_t

        def sd_of(q_t, mu, s_t):
            var = np.maximum((-2 * mu * s_t + sw_t * mu ** 2 + q_t) / divisor, 0)
            sd = np.sqrt(var)
            return np.where(sd <= resolution, 1, sd)
        if mean_X or std_X:
            sX_t = (tot["s"] - upd["s"]).reshape(1, -1)
            muX = sX_t / sw_t
            if std_X:
                sdX = sd_of((tot["q"] - upd["q"]).reshape(1, -1), muX, sX_t)
        if mean_Y or std_Y:
            sY_t = (tot["sy"] - upd["sy"]).reshape(1, -1)
            muY = sY_t / sw_t
            if std_Y:
                sdY = sd_of((tot["qy"] - upd["qy"]).reshape(1, -1), muY, sY_t)

    def kernel(total, u, muA, muB, sdA, sdB, center):
        out = total - u
        if center:
            out = out - sw_t * (muA.T @ muB)
        if sdA is not None and sdB is not None:
            out = out / (sdA.T @ sdB)
        elif sdA is not None:
            out = out / sdA.T
        elif sdB is not None:
            out = out / sdB
        return out.astype(dt)
    xtx = kernel(tot["U"], upd["U"], muX, muX, sdX, sdX, cX) if rXTX else None
    xty = kernel(tot["V"], upd["V"], muX, muY, sdX, sdY, cX or cY) if rXTY else None
    r = lambda a, keep: a.astype(dt) if (a is not None and keep) else None      # noqa: E731
    stats = (r(muX, mean_X), r(sdX, std_X), r(muY, mean_Y), r(sdY, std_Y))
    return ((xtx, xty) if rXTX and rXTY else (xtx if rXTX else xty)), stats


def union_update(acc, S):
    return {k: sum((acc[f][k] for f in sorted(S)[1:]), acc[sorted(S)[0]][k] * 1.0) for k in ("U", "V", "s", "q", "sy", "qy", "sw", "nz")}


def model_folds(X, Y, w, labels, rows, flags, method, dt=np.float64, ddof=1, P=uc.P):
    acc = accumulate(X, Y, w, labels, rows, P, dt)
    tot = close(acc, dt)
    out = []
    for f in range(P):
        try:
            out.append(finish(tot, acc[f], flags, method, ddof, dt, w is not None, Y is not None))
        except ValueError as e:
            out.append(str(e))
    return out


# ---------------------------------------------------------------- the gates, on the GPU test's grid
@pytest.mark.parametrize("chunking", sc.CHUNKINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", uc.SHAPES)
def test_model_float64_parity(K, M, weighted, chunking):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    rows = sc.chunk_rows(chunking, labels)
    for flags in uc.FLAGS:
        for method in (uc.METHODS if M is not None else ("XTX",)):
            refs = sc.fold_reference(K, M, weighted, flags, method)
            got = model_folds(X, Y, w, labels, rows, flags, method)
            for f in range(uc.P):
                what = f"K={K} M={M} w={weighted} {chunking} flags={flags} {method} fold {f}"
                if isinstance(refs[f], str):
                    assert got[f] == refs[f], what
                    continue
                gx, gy, gstats = uc.split_result(method, got[f])
                rx, ry, rstats = uc.split_result(method, refs[f])
                if rx is not None:
                    assert_normwise(gx, rx, TOL, what + " XTX")
                if ry is not None:
                    assert_normwise(gy, ry, TOL, what + " XTY")
                assert_stats(gstats, rstats, TOL, what)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", uc.SHAPES)
def test_model_unions(K, M, weighted):
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    rows = sc.chunk_rows("B", labels)
    acc = accumulate(X, Y, w, labels, rows, uc.P, np.float64)
    tot = close(acc, np.float64)
    for flags in uc.FLAGS:
        for method in (uc.METHODS if M is not None else ("XTX",)):
            refs = uc.base_reference(K, M, weighted, flags, method)
            for u, S in enumerate(uc.UNIONS):
                what = f"K={K} M={M} w={weighted} flags={flags} {method} union {S}"
                try:
                    got = finish(tot, union_update(acc, S), flags, method, 1, np.float64, weighted, Y is not None)
                except ValueError as e:
                    assert str(e) == refs[u], what
                    continue
                assert not isinstance(refs[u], str), what
                gx, gy, gstats = uc.split_result(method, got)
                rx, ry, rstats = uc.split_result(method, refs[u])
                if uc.weightless(weighted, S):                   # (exactly zero matrices: the scale of the operands)
                    sx, sy = uc.full_scale(K, M, weighted)
                    assert rx is None or np.abs(gx - rx).max() <= TOL * sx, what
                    assert ry is None or np.abs(gy - ry).max() <= TOL * sy, what
                    continue
                if rx is not None:
                    assert_normwise(gx, rx, TOL, what + " XTX")
                if ry is not None:
                    assert_normwise(gy, ry, TOL, what + " XTY")
                assert_stats(gstats, rstats, TOL, what)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,M", [(64, 3), (130, 3)])
def test_model_float32_within_the_gate(K, M, weighted):
    from cvmatrix_amd.fp32_gate import fp32_bound
    X, Y, w, labels, folds = uc.base_design(K, M, weighted)
    rows = sc.chunk_rows("B", labels)
    for flags in uc.FLAGS:
        ref64, ref32 = sc.fold_reference32(K, M, weighted, flags)
        got = model_folds(X, Y, w, labels, rows, flags, "XTX_XTY", np.float32)
        for f in range(uc.P):
            if isinstance(ref64[f], str) or isinstance(ref32[f], str):
                assert got[f] == ref64[f]
                continue
            for i, name in enumerate(("XTX", "XTY")):
                err, yard = sc.fp32_errors(got[f][0][i], ref64[f][0][i], ref32[f][0][i])
                assert err <= fp32_bound(yard), (K, weighted, flags, f, name, err, yard)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_model_two_chunks_of_the_split_design(dtype_name):
    from cvmatrix_amd.fp32_gate import fp32_bound
    X, Y, w, labels, folds = uc.split_design(dtype_name)
    rows = [np.arange(0, 600), np.arange(600, 1200)]
    dt = np.dtype(dtype_name).type
    for flags in ((True,) * 4, (False,) * 4):
        ref64, refdt = sc.split_reference(dtype_name, flags)
        got = model_folds(X.astype(np.float64), Y.astype(np.float64), w.astype(np.float64), labels, rows, flags,
                          "XTX_XTY", dt, P=5)
        for f in range(5):
            for i, name in enumerate(("XTX", "XTY")):
                if dt is np.float64:
                    assert_normwise(got[f][0][i], ref64[f][0][i], TOL, f"{flags} fold {f} {name}")
                else:
                    err, yard = sc.fp32_errors(got[f][0][i], ref64[f][0][i], refdt[f][0][i])
                    assert err <= fp32_bound(yard), (flags, f, name, err, yard)
            if dt is np.float64:
                assert_stats(got[f][1], ref64[f][1], TOL, f"{flags} fold {f}")


def test_chunkings_cover_every_row_once():
    _, _, _, labels, _ = uc.base_design(7, 1, False)
    for name in sc.CHUNKINGS:
        rows = sc.chunk_rows(name, labels)
        assert sorted(np.concatenate(rows).tolist()) == list(range(uc.N)), name
    assert [len(r) for r in sc.chunk_rows("B", labels)] == [80, 0, 1, 122]
    assert all(len(set(labels[r].tolist())) == 1 for r in sc.chunk_rows("C", labels))
    assert any(len(set(labels[r].tolist())) < uc.P for r in sc.chunk_rows("B", labels))


# ---------------------------------------------------------------- argument rules that need no device
def test_chunk_rules():
    from cvmatrix_amd.streaming import ChunkRules
    r = ChunkRules(5)
    X, Y, w, lab = np.zeros((4, 7)), np.zeros((4, 2)), np.ones(4), np.array([0, 4, 2, 2])
    out, K, M = r.check(X, Y, w, lab)
    assert (K, M) == (7, 2) and out.dtype == np.int64 and out.tolist() == lab.tolist()
    assert r.check(X[:, 0], None, None, lab)[1:] == (1, None)                    # 1-D: one column
    for bad in ([0, 5, 1, 1], [-1, 0, 0, 0], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            r.check(X, Y, w, np.array(bad))
    with pytest.raises(ValueError):
        r.check(X, Y, w, None)
    with pytest.raises(ValueError):
        r.check(X, Y, w, lab[:3])                                                # rows of X and labels differ
    with pytest.raises(ValueError):
        r.check(X, Y[:3], w, lab)
    with pytest.raises(ValueError):
        r.check(X, Y, np.ones((4, 2)), lab)
    r.fix(7, 2, True, True)
    r.check(X, Y, w, lab)
    r.check(X[:0], Y[:0], w[:0], lab[:0])                                        # an empty chunk of the right shape
    for args in ((np.zeros((4, 8)), Y, w), (X, None, w), (X, np.zeros((4, 3)), w), (X, Y, None)):
        with pytest.raises(ValueError):
            r.check(*args, lab)
    r2 = ChunkRules(5)
    r2.fix(7, None, False, False)
    for args in ((X, Y, None), (X, None, w)):
        with pytest.raises(ValueError):
            r2.check(*args, lab)


def test_streaming_object_rules_without_a_device():
    import cvmatrix_amd
    from cvmatrix_amd.cvmatrix import MSG_NEG_W
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            cvmatrix_amd.StreamingCVMatrix(bad)
    with pytest.raises(TypeError):
        cvmatrix_amd.StreamingCVMatrix(3, dtype=np.int32)
    scv = cvmatrix_amd.StreamingCVMatrix(3, True, True)
    assert scv.N == 0 and scv.n_chunks == 0 and scv.accumulator_bytes == 0 and scv.fold_sizes.tolist() == [0, 0, 0]
    X = np.zeros((2, 4))
    with pytest.raises(ValueError):
        scv.partial_fit(X, None, None, [0, 3])                                   # a label out of range
    with pytest.raises(ValueError) as e:
        scv.partial_fit(X, None, np.array([1.0, -1.0]), [0, 1])                  # a negative host weight
    assert str(e.value) == MSG_NEG_W
    scv.partial_fit(X[:0], None, None, np.zeros(0, dtype=np.int64))              # an empty chunk: a no-op
    assert scv.N == 0 and scv.n_chunks == 0 and scv.K is None
    for call in (scv.training_XTX_batched, scv.training_XTX_XTY_batched, scv.training_statistics_batched,
                 lambda: scv.training_XTX_unions([[0, 1]]), lambda: scv.XTX):
        with pytest.raises(RuntimeError):
            call()
    assert scv.sum_X is None and scv.sum_w is None and scv.num_nonzero_w is None


def test_exports_and_header():
    import os
    from cvmatrix_amd import _lib
    names = ("cvm_stream_workspace_bytes", "cvm_stream_reset", "cvm_stream_add", "cvm_stream_close")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvmhip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and n + "(" in header
