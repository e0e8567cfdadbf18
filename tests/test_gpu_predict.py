"""GPU (-m gpu): the device predictions (cvm_cv_predict through cv_predict, predict and the C ABI) against the
reference and the gate of tests/predict_cases.py, whose own conditions tests/test_predict_host.py checks on
the CPU.  The gate is derived there, not calibrated; every test prints where the kernel lands (run with -s).
The largest ratio |out - ref| / gate seen on the MI355X:
  test_shape_grid                float64  0.49 (K = 1), 0.34 (K = 3), 0.27 (K = 4), falling to 0.02 at K = 130
                                 float32  0.47 (K = 1), 0.34 (K = 3), 0.31 (K = 4), falling to 0.02 at K = 130
  test_every_combination_of_statistics    0.08 in both dtypes
  test_an_empty_fold 0.12, test_more_folds_than_a_grid_dimension 0.26 (K = 4, 65539 predictions)
  test_end_to_end                0.12 at most (K = 13, a padded X)
  test_agreement_with_the_scorer 0.02 of its bound
(The short K come closest: of the K + 8 roundings the gate allows, the eight of the standardisation and the
epilogue are the ones a short sum really makes.)"""

import itertools

import numpy as np
import pytest
import torch

import predict_cases as pc

pytestmark = pytest.mark.gpu

DT = {"float64": np.float64, "float32": np.float32}


@pytest.fixture(scope="module")
def pm(hip_device):
    pc.require_longdouble()
    from cvmatrix_amd import _lib
    _lib.load()
    from cvmatrix_amd import predict as mod
    return mod


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def devs(stats):
    return tuple(dev(s) for s in stats)


def host(t):
    return t.cpu().numpy()


def model(X, Y=None, w=None, dtype=np.float64, **kw):
    from cvmatrix_amd import CVMatrix
    cvm = CVMatrix(dtype=dtype, **kw)
    cvm.fit(X, Y, w)
    return cvm


def run_predict(pm, X, B, stats=None):
    return host(pm.predict(dev(X), dev(B), None if stats is None else devs(stats)))


# ------------------------------------------------------------------------------------------ shape grid
@pytest.mark.parametrize("K", pc.GRID_K)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_shape_grid(pm, dtype, K):
    """Ragged folds of 1, 63, 64, 65 and 129 rows in one batch, every (A, M) of the grid: cv_predict in both
    orders and predict fold by fold, against the reference within the gate."""
    rng = np.random.default_rng(7 * K + (dtype == "float32"))
    folds, N = pc.ragged_folds(rng)
    F = len(folds)
    worst = 0.0
    for A, M in pc.GRID_AM[dtype]:
        X, B, stats = pc.design(rng, N, K, A, M, DT[dtype], F=F)       # (statistics near THIS X's own)
        cvm = model(X, dtype=DT[dtype])
        assert pc.same_bits(host(cvm.X), X)                            # the values the device reads
        ref, gate = pc.cv_reference(X, folds, B, stats)
        out = host(pm.cv_predict(cvm, folds, devs(stats), dev(B), order="folds"))
        worst = max(worst, pc.assert_gate(out, ref, gate, f"cv_predict {dtype} K = {K} A = {A} M = {M}"))
        rows = host(pm.cv_predict(cvm, folds, devs(stats), dev(B)))
        assert pc.same_bits(rows[np.concatenate(folds)], out)
        p = 0
        for f, v in enumerate(folds):
            one = run_predict(pm, X[v], B[f], pc.fold_stats(stats, f))
            assert pc.worst_ratio(one, ref[p:p + v.size], gate[p:p + v.size]) <= 1.0
            assert pc.same_bits(one, out[p:p + v.size]), (A, M, f)
            p += v.size
    print(f"test_shape_grid {dtype} K = {K}: at most {worst:.3f} of the gate")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_combination_of_statistics(pm, dtype):
    rng = np.random.default_rng(11)
    worst = 0.0
    for mask in itertools.product((False, True), repeat=4):
        X, B, stats = pc.design(rng, 70, 17, 3, 5, DT[dtype], mask)
        ref, gate = pc.reference(X, B, stats)
        worst = max(worst, pc.assert_gate(run_predict(pm, X, B, stats), ref, gate, f"{dtype} statistics {mask}"))
    print(f"test_every_combination_of_statistics {dtype}: at most {worst:.3f} of the gate")


# ------------------------------------------------------------------------------------------ C ABI
def cabi(X, idx, offsets, max_rows, B, stats, n_out, by_row=0):
    from cvmatrix_amd import _lib
    lib = _lib.load()
    F, A, K, M = B.shape
    out = torch.full((n_out, A, M), float("nan"), dtype=X.dtype, device=X.device)
    code = _lib.CVM_F64 if X.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_cv_predict(_lib.ptr(X), X.stride(0), _lib.ptr(idx), _lib.ptr(offsets), F, max_rows, K, M, A, code,
                            *(_lib.ptr(s) for s in stats), _lib.ptr(B), _lib.ptr(out), by_row,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.CVM_OK, lib.cvm_last_error()
    torch.cuda.synchronize()
    return host(out)


def test_an_empty_fold(pm):
    rng = np.random.default_rng(21)
    sizes = (5, 0, 70, 0)
    folds, N = pc.ragged_folds(rng, sizes)
    X, B, stats = pc.design(rng, N, 6, 2, 3, np.float64, F=len(sizes))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = cabi(dev(X), dev(np.concatenate(folds)), dev(offsets), max(sizes), dev(B), devs(stats), N)
    ref, gate = pc.cv_reference(X, folds, B, stats)
    pc.assert_gate(out, ref, gate, "an empty fold between two others and one at the end")
    # every fold empty: nothing is read, nothing is written
    none = cabi(dev(X), dev(np.zeros(0, np.int64)), dev(np.zeros(5, np.int64)), 0, dev(B), devs(stats), 3)
    assert np.isnan(none).all()


def test_more_folds_than_a_grid_dimension(pm):
    """F = 65539 folds of one row each, K = 4, A = M = 1: every prediction."""
    rng = np.random.default_rng(22)
    F, K = 65539, 4
    X, B, stats = pc.design(rng, F, K, 1, 1, np.float64, F=F)
    perm = rng.permutation(F).astype(np.int64)
    out = cabi(dev(X), dev(perm), dev(np.arange(F + 1, dtype=np.int64)), 1, dev(B), devs(stats), F)
    ref, gate = pc.one_row_fold_reference(X[perm], B, stats)
    pc.assert_gate(out[:, 0, 0], ref, gate, "65539 folds of one row")
    # the same folds by row number
    rows = cabi(dev(X), dev(perm), dev(np.arange(F + 1, dtype=np.int64)), 1, dev(B), devs(stats), F, by_row=1)
    assert pc.same_bits(rows[perm], out)
    # more workgroups than one launch may have: with the longest fold given as 16384 rows (an upper bound does no
    # harm: the chunks past a fold's end leave at once) the plan has 65539 x 256 of them, cut inside fold 65535
    from cvmatrix_amd import _lib
    info = np.zeros(9, dtype=np.int64)
    assert _lib.load().cvm_cv_predict_plan(F, 16384, K, K, 1, 1, _lib.CVM_F64, 1, info.ctypes.data) == _lib.CVM_OK
    assert info[3] == F * 256 > 2 ** 24 - 1 and info[4] == 2 and info[5] == 2 ** 24 - 1
    cut = cabi(dev(X), dev(perm), dev(np.arange(F + 1, dtype=np.int64)), 16384, dev(B), devs(stats), F)
    assert pc.same_bits(cut, out)


# ------------------------------------------------------------------------------------------ end to end
FLAGS = ((True, True, True, True), (True, True, False, False), (False, False, False, False), (True, False, True, False))


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(31)
    N, K, M = 301, 13, 3
    L = rng.normal(size=(N, 4)) * np.array([5.0, 3.0, 2.0, 1.0])
    X = L @ rng.normal(size=(4, K)) + 0.3 * rng.normal(size=(N, K)) + rng.normal(size=K) * 2
    Y = L[:, :2] @ rng.normal(size=(2, M)) + 0.1 * rng.normal(size=(N, M)) + 4
    w = rng.uniform(0.2, 2.0, N)
    labels = rng.integers(0, 5, N)
    folds = [np.flatnonzero(labels == f).astype(np.int64) for f in range(5)]
    return X, Y, w, folds


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "".join("ft"[b] for b in f))
def test_end_to_end(pm, problem, flags, weighted):
    """CVMatrix -> a fitter -> cv_predict, for the three fitters (K = 13, M = 3 in float64: X and Y both padded,
    the row pitch of X is 14)."""
    from cvmatrix_amd.pcr import pcr_fit_batched
    from cvmatrix_amd.pls import pls_fit_batched
    from cvmatrix_amd.ridge import ridge_fit_batched
    X, Y, w, folds = problem
    cx, cy, sx, sy = flags
    cvm = model(X, Y, w if weighted else None, center_X=cx, center_Y=cy, scale_X=sx, scale_Y=sy)
    assert cvm.X.stride(0) == 14
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    Xd = host(cvm.X)
    hstats = tuple(None if s is None else host(s) for s in stats)
    worst = 0.0
    for name, B in (("pls", pls_fit_batched(XTX, XTY, 4).B), ("ridge", ridge_fit_batched(XTX, XTY, [0.0, 0.1, 10.0]).B),
                    ("pcr", pcr_fit_batched(XTX, XTY, 5).B)):
        out = host(pm.cv_predict(cvm, batch, stats, B, order="folds"))
        ref, gate = pc.cv_reference(Xd, folds, host(B), hstats)
        worst = max(worst, pc.assert_gate(out, ref, gate, f"{name} {flags} weighted {weighted}"))
        rows = host(pm.cv_predict(cvm, batch, stats, B))
        assert pc.same_bits(rows[np.concatenate(folds)], out)
    print(f"test_end_to_end {flags} weighted {weighted}: at most {worst:.3f} of the gate")


def test_agreement_with_the_scorer(pm):
    """sum_i w_i e_i^2 of the predictions against pls_validation_sse (an unpadded float64 model): within what
    the elementwise gate g lets the squares move, plus the scorer's own float64 sum:
    |sum w e^2 - sse| <= sum w (2 |e| g + g^2) + (n + 4) 2^-53 sse."""
    from cvmatrix_amd.pls import pls_fit_batched, pls_validation_sse
    rng = np.random.default_rng(41)
    N, K, M, A = 420, 16, 4, 5
    X = rng.normal(size=(N, K)) * rng.uniform(0.5, 3, K) + rng.normal(size=K)
    Y = X @ rng.normal(size=(K, M)) * 0.2 + 0.5 * rng.normal(size=(N, M)) + 2
    w = rng.uniform(0.1, 3.0, N)
    folds, _ = pc.ragged_folds(rng, (1, 63, 64, 65, 129, 98))
    cvm = model(X, Y, w)
    assert cvm._Kd == cvm._Ku and cvm._Md == cvm._Mu
    batch = cvm.prepare_folds(folds)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    B = pls_fit_batched(XTX, XTY, A).B
    sse, wsum = pls_validation_sse(cvm, batch, stats, B)
    sse = host(sse).astype(pc.LD)
    out = host(pm.cv_predict(cvm, batch, stats, B, order="folds")).astype(pc.LD)
    _, gate = pc.cv_reference(host(cvm.X), folds, host(B), tuple(host(s) for s in stats))
    Yd, wd = host(cvm.Y).astype(pc.LD), host(cvm.weights).reshape(-1).astype(pc.LD)
    p, worst = 0, 0.0
    for f, v in enumerate(folds):
        e = out[p:p + v.size] - Yd[v][:, None, :]
        g = gate[p:p + v.size]
        wv = wd[v][:, None, None]
        mine = (wv * e * e).sum(axis=0)
        bound = (wv * (2 * np.abs(e) * g + g * g)).sum(axis=0) + (v.size + 4) * pc.LD(2.0 ** -53) * sse[f]
        d = np.abs(mine - sse[f])
        assert (d <= bound).all(), (f, float((d / bound).max()))
        worst = max(worst, float((d / bound).max()))
        p += v.size
    print(f"test_agreement_with_the_scorer: at most {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------ bitwise properties
@pytest.fixture(scope="module")
def batch64(pm):
    """One float64 model with ragged folds, 7 rows in no fold, and its predictions (A = 3, M = 4, K = 16)."""
    rng = np.random.default_rng(51)
    folds, N = pc.ragged_folds(rng, extra=7)
    X, B, stats = pc.design(rng, N, 16, 3, 4, np.float64, F=len(folds))
    cvm = model(X)
    dB, dst = dev(B), devs(stats)
    by_fold = host(pm.cv_predict(cvm, folds, dst, dB, order="folds"))
    by_row = host(pm.cv_predict(cvm, folds, dst, dB))
    return dict(cvm=cvm, folds=folds, N=N, X=X, B=B, stats=stats, dB=dB, dst=dst, by_fold=by_fold, by_row=by_row)


def test_orders_agree_and_uncovered_rows_are_nan(pm, batch64):
    b = batch64
    idx = np.concatenate(b["folds"])
    assert pc.same_bits(b["by_row"][idx], b["by_fold"])
    rest = np.setdiff1d(np.arange(b["N"]), idx)
    assert rest.size == 7 and np.isnan(b["by_row"][rest]).all()
    assert np.isfinite(b["by_fold"]).all()


def test_a_fold_is_predict_on_its_rows(pm, batch64):
    b = batch64
    p = 0
    for f, v in enumerate(b["folds"]):
        one = host(pm.predict(b["cvm"].X[dev(v)], b["dB"][f], tuple(s[f] for s in b["dst"])))
        assert pc.same_bits(one, b["by_fold"][p:p + v.size]), f
        p += v.size


def test_fold_order_and_batch_do_not_matter(pm, batch64):
    b = batch64
    rev = host(pm.cv_predict(b["cvm"], b["folds"][::-1], tuple(s.flip(0) for s in b["dst"]), b["dB"].flip(0)))
    assert pc.same_bits(rev, b["by_row"])
    p = 0
    for f, v in enumerate(b["folds"]):
        alone = host(pm.cv_predict(b["cvm"], [v], tuple(s[f:f + 1] for s in b["dst"]), b["dB"][f:f + 1], order="folds"))
        assert pc.same_bits(alone, b["by_fold"][p:p + v.size]), f
        p += v.size


# (dtype, K, A, M, the narrower M): the full call and its slices on both sides of every route decision of
# the host code -- column tiles per wave (A M against 64, 128, ... and the widest variant), statistics in LDS
# (K against 512 under a narrow variant; a wide variant keeps them in LDS beyond), 16-byte loads (K and M
# against the vector width)
SLICES = (("float64", 16, 6, 16, 3), ("float64", 520, 5, 4, 2), ("float64", 520, 5, 4, 1), ("float64", 520, 80, 4, 2),
          ("float64", 18, 9, 8, 4), ("float32", 36, 24, 16, 5), ("float32", 520, 6, 8, 4), ("float32", 34, 96, 4, 1),
          ("float64", 17, 41, 8, 2))


@pytest.mark.parametrize("dtype,K,A,M,Mn", SLICES)
def test_columns_do_not_depend_on_their_neighbours(pm, dtype, K, A, M, Mn):
    rng = np.random.default_rng(K + A)
    X, B, stats = pc.design(rng, 70, K, A, M, DT[dtype])
    full = run_predict(pm, X, B, stats)
    for a in sorted({0, A // 2, A - 1}):
        assert pc.same_bits(run_predict(pm, X, B[a:a + 1], stats), full[:, a:a + 1]), a
    for m0 in sorted({0, M - Mn}):
        st = (stats[0], stats[1], stats[2][m0:m0 + Mn], stats[3][m0:m0 + Mn])
        part = run_predict(pm, X, np.ascontiguousarray(B[:, :, m0:m0 + Mn]), st)
        assert pc.same_bits(part, full[:, :, m0:m0 + Mn]), m0
    # the other rows do not matter either: one row alone, and the rows in another order
    assert pc.same_bits(run_predict(pm, X[33:34], B, stats), full[33:34])
    perm = rng.permutation(70)
    assert pc.same_bits(run_predict(pm, X[perm], B, stats), full[perm])


@pytest.mark.parametrize("dtype,K,M", [("float64", 35, 3), ("float32", 130, 2)])
def test_a_padded_model_is_the_unpadded_one(pm, dtype, K, M):
    from cvmatrix_amd.pls import pls_fit_batched
    rng = np.random.default_rng(61)
    folds, N = pc.ragged_folds(rng, (40, 64, 27, 90))
    X = (rng.normal(size=(N, K)) + rng.normal(size=K)).astype(DT[dtype])
    Y = (X[:, :5] @ rng.normal(size=(5, M)) + 0.1 * rng.normal(size=(N, M))).astype(DT[dtype])
    padded = model(X, Y, dtype=DT[dtype])
    assert padded.X.stride(0) > K                               # (what this test is about)
    (XTX, XTY), stats = padded.training_XTX_XTY_batched(folds)
    B = pls_fit_batched(XTX, XTY, 3).B
    plain = model(dev(X), dev(Y), dtype=DT[dtype], copy=False)
    assert plain.X.stride(0) == K
    for order in ("rows", "folds"):
        a = host(pm.cv_predict(padded, folds, stats, B, order=order))
        assert np.isfinite(a).all()
        assert pc.same_bits(a, host(pm.cv_predict(plain, folds, stats, B, order=order))), order


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_alignment_and_row_pitch_do_not_matter(pm, dtype):
    rng = np.random.default_rng(71)
    n, K, A, M = 70, 16, 5, 4
    X, B, stats = pc.design(rng, n, K, A, M, DT[dtype])
    dst = devs(stats)
    full = host(pm.predict(dev(X), dev(B), dst))
    # X and B one element into a larger buffer: no 16-byte loads
    bx = torch.zeros(n * K + 1, dtype=dev(X).dtype, device="cuda")
    bb = torch.zeros(A * K * M + 1, dtype=bx.dtype, device="cuda")
    bx[1:].copy_(dev(X).reshape(-1))
    bb[1:].copy_(dev(B).reshape(-1))
    Xv, Bv = bx[1:].view(n, K), bb[1:].view(A, K, M)
    assert Xv.data_ptr() % 16 != 0 and Bv.data_ptr() % 16 != 0 and Bv.is_contiguous()
    assert pc.same_bits(host(pm.predict(Xv, Bv, dst)), full)
    assert pc.same_bits(host(pm.predict(Xv, dev(B), dst)), full)
    assert pc.same_bits(host(pm.predict(dev(X), Bv, dst)), full)
    # rows of a wider matrix: a pitch of K + 4 (16-byte loads stay) and of K + 1 (they do not)
    for extra in (4, 1):
        wide = torch.zeros((n, K + extra), dtype=bx.dtype, device="cuda")
        wide[:, :K].copy_(dev(X))
        assert pc.same_bits(host(pm.predict(wide[:, :K], dev(B), dst)), full), extra


def test_out_and_stream_do_not_matter(pm, batch64):
    b = batch64
    for order, want in (("rows", b["by_row"]), ("folds", b["by_fold"])):
        buf = torch.empty(want.shape, dtype=torch.float64, device="cuda")
        got = pm.cv_predict(b["cvm"], b["folds"], b["dst"], b["dB"], order=order, out=buf)
        assert got is buf and pc.same_bits(host(buf), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = pm.cv_predict(b["cvm"], b["folds"], b["dst"], b["dB"])
        one = pm.predict(dev(b["X"]), b["dB"][0], tuple(t[0] for t in b["dst"]))
    s.synchronize()
    assert pc.same_bits(host(got), b["by_row"])
    assert pc.same_bits(host(one)[b["folds"][0]], b["by_fold"][:b["folds"][0].size])


# ------------------------------------------------------------------------------------------ containment
def test_a_nan_fold_stays_a_nan_fold(pm, batch64):
    b = batch64
    B = b["dB"].clone()
    B[3] = float("nan")                      # (what the fitters leave for a fold with non-finite input)
    got = host(pm.cv_predict(b["cvm"], b["folds"], b["dst"], B))
    bad = b["folds"][3]
    assert np.isnan(got[bad]).all()
    keep = np.setdiff1d(np.arange(b["N"]), bad)
    assert pc.same_bits(got[keep], b["by_row"][keep])


def test_a_nan_in_one_row_stays_in_that_row(pm, batch64):
    b = batch64
    row = int(b["folds"][4][77])
    for col in (0, 9, 15):
        X = b["X"].copy()
        X[row, col] = np.nan
        cvm = model(X)
        got = host(pm.cv_predict(cvm, b["folds"], b["dst"], b["dB"]))
        assert np.isnan(got[row]).all()
        keep = np.setdiff1d(np.arange(b["N"]), [row])
        assert pc.same_bits(got[keep], b["by_row"][keep]), col


def test_a_row_in_two_folds(pm, batch64):
    b = batch64
    folds = [f.copy() for f in b["folds"]]
    folds[1] = np.concatenate([folds[1], folds[2][:1]])
    B = b["dB"]
    with pytest.raises(ValueError, match="more than one fold"):
        pm.cv_predict(b["cvm"], folds, b["dst"], B)
    # by position the folds may overlap: the shared row once under each model
    out = host(pm.cv_predict(b["cvm"], folds, b["dst"], B, order="folds"))
    assert out.shape[0] == sum(f.size for f in folds) and np.isfinite(out).all()
    sizes = np.cumsum([0] + [f.size for f in folds])
    row = int(folds[2][0])
    assert pc.same_bits(out[sizes[2]], b["by_row"][row])
    alone = host(pm.predict(b["cvm"].X[row:row + 1], b["dB"][1], tuple(s[1] for s in b["dst"])))
    assert pc.same_bits(out[sizes[2] - 1:sizes[2]], alone)


# ------------------------------------------------------------------------------------------ argument errors
def test_cv_predict_argument_errors(pm, batch64):
    b = batch64
    cvm, folds, dst, B = b["cvm"], b["folds"], b["dst"], b["dB"]
    bad = [
        dict(B=B[:4]), dict(B=B[:, :, :15]), dict(B=B[0]), dict(B=B.float()), dict(order="columns"),
        dict(stats=dst[:3]), dict(stats=(dst[0][:4],) + dst[1:]), dict(stats=(dst[0].float(),) + dst[1:]),
        dict(stats=dst[:2] + (dst[2][:, :3], dst[3])),
        dict(stats=(dst[0].t().contiguous(),) + dst[1:]), dict(stats=(dst[0].reshape(-1),) + dst[1:]),
        dict(out=torch.empty((b["N"], 3, 5), dtype=torch.float64, device="cuda")),
        dict(out=torch.empty((b["N"], 3, 4), dtype=torch.float32, device="cuda")),
        dict(out=torch.empty((b["N"], 3, 8), dtype=torch.float64, device="cuda")[:, :, ::2]),
        dict(out=torch.empty((b["N"] - 7, 3, 4), dtype=torch.float64, device="cuda")),
    ]
    for kw in bad:
        a = dict(stats=dst, B=B, order="rows", out=None)
        a.update(kw)
        with pytest.raises(ValueError):
            pm.cv_predict(cvm, folds, a["stats"], a["B"], order=a["order"], out=a["out"])
    with pytest.raises(TypeError):
        pm.cv_predict(cvm, folds, dst, B, out=torch.empty((b["N"], 3, 4), dtype=torch.float64))
    with pytest.raises(TypeError):
        pm.cv_predict(cvm, folds, (dst[0].cpu(),) + dst[1:], B)
    # models whose results are not device tensors of the computing dtype
    for kw in (dict(output="numpy"), dict(dtype=np.float16)):
        other = model(b["X"], **kw)
        with pytest.raises(ValueError):
            pm.cv_predict(other, folds, dst, B)


def test_predict_argument_errors(pm):
    X = torch.ones((6, 8), dtype=torch.float64, device="cuda")
    B = torch.ones((2, 8, 3), dtype=torch.float64, device="cuda")
    v8, v3 = torch.ones(8, dtype=torch.float64, device="cuda"), torch.ones(3, dtype=torch.float64, device="cuda")
    assert pm.predict(X, B, (v8, v8, v3, v3)).shape == (6, 2, 3)
    assert pm.predict(X, B[0]).shape == (6, 1, 3)
    assert pm.predict(X[:0], B).shape == (0, 2, 3)
    for args in ((X[:, :7], B), (X[0], B), (X, B.unsqueeze(0)), (X.float(), B), (X.t().contiguous().t(), B),
                 (X, torch.ones((2, 8, 65), dtype=torch.float64, device="cuda")),
                 (X, B, (v8, v8, v3)), (X, B, (v3, v8, v3, v3)), (X, B, (v8, v8, v8, v3)),
                 (X, B, (v8.float(), v8, v3, v3)), (X, B, (v8.reshape(1, 8), v8, v3, v3))):
        with pytest.raises(ValueError):
            pm.predict(*args)
    with pytest.raises(TypeError):
        pm.predict(X, B, (v8.cpu(), v8, v3, v3))
