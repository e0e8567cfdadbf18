"""GPU (-m gpu): the validation scorer (cvm_pls_validation_sse through the C ABI and pls.pls_validation_sse)
against the np.longdouble reference and the derived gate of tests/sse_cases.py, whose own conditions
tests/test_sse_host.py checks on the CPU -- every column of every fold, not the fold's largest value -- and the
scorer's contract as include/cvmhip.h states it: limits, empty folds, which inputs a fold's bits depend on,
where values that are not finite end up.  Inputs are formed by NumPy and uploaded: the device and the reference
read the same bits.  Through the C ABI the workspace has exactly cvm_pls_sse_workspace_bytes bytes, filled with
NaN bytes, and the outputs are filled with a sentinel.  Every test prints where the kernel lands (run with -s).
The largest |sse - sse_ref| / gate seen on the MI355X:
  test_shape_grid    float64  0.29 (K = 1), 0.25 (K = 3), 0.19 (K = 4), 0.05 .. 0.08 (K = 15 .. 17), 0.03 (K = 33),
                              0.011 (K = 130)
                     float32  0.08 (K = 1), 0.10 (K = 3), 0.07 (K = 4), 0.03 .. 0.04 (K = 15 .. 17), 0.02 (K = 33),
                              0.008 (K = 130)
  test_every_variant_and_both_places_of_the_statistics
                     float64  0.042 (K = 20 / 21: 0.02 .. 0.04; K = 520 / 521: 0.001 .. 0.002)
                     float32  0.055 (K = 20 / 21: 0.02 .. 0.05; K = 520 / 521: 0.001 .. 0.003)
  test_every_combination_of_statistics_and_weights   float64 0.049 (K = 17), 0.034 (K = 16); float32 0.033, 0.044
  test_hard_values   float64 0.020 (K = 33), 0.006 (K = 36); float32 0.013, 0.003
  the batch of the bit tests and test_a_row_in_two_folds   0.028 (float64, K = 20), 0.001 (K = 520), 0.010
                     (float32, K = 36), 0.001 (K = 520)
  test_zero_weights_and_empty_folds   float64 0.041, float32 0.013
  test_the_most_folds_one_call_takes  0.23 (K = 4, 65535 sums of one term)
(As for the predictions the short K come closest -- of the K + 8 roundings the gate allows, the eight of the
standardisation and the epilogue are the ones a short sum really makes -- and float32 lies further inside than
float64 because its epilogue runs in float64.  The emulation of tests/test_sse_host.py lies at 0.0002 .. 0.016.)
The library before this file failed test_statistics_that_are_not_finite_make_the_fold_non_finite at K = 20 for
sdX = +inf and -inf in both dtypes: with the statistics in LDS the reciprocal was 1.0 / sd = 0, z = 0, and the
fold's twelve sums were finite numbers that ignored the column (ScorerRcp::lds now gives NaN there; finite sd:
the same bits, profiles/sse_contract/).  Everything else passed as it stood."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import predict_cases as pc
import sse_cases as sc

pytestmark = pytest.mark.gpu

DT = {"float64": np.float64, "float32": np.float32}
SENTINEL = -7.25e77
RAGGED = (1, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def lib(hip_device):
    pc.require_longdouble()
    from cvmatrix_amd import _lib
    return _lib.load()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def upload(d):
    return dict(X=dev(d["X"]), Y=dev(d["Y"]), w=dev(d["w"]), B=dev(d["B"]), stats=tuple(dev(s) for s in d["stats"]))


def untouched(a):
    return bool((a == SENTINEL).all())


def score(lib, X, Y, w, folds, B, stats, *, max_rows=None, ws_fill=0xFF, n_folds=None, n_out=None, ws_short=0, want=0):
    """cvm_pls_validation_sse on device tensors, `folds` a list of index arrays.  Returns (sse (n_out, A, M), wsum
    (n_out,)) as NumPy arrays: the rows past n_folds keep the sentinel."""
    from cvmatrix_amd import _lib
    _, A, K, M = B.shape
    F = len(folds) if n_folds is None else n_folds
    sizes = [int(v.size) for v in folds]
    idx = dev(np.concatenate(folds).astype(np.int64)) if sum(sizes) else None
    offsets = dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    if max_rows is None:
        max_rows = max(sizes, default=0)
    nbytes = lib.cvm_pls_sse_workspace_bytes(F, max_rows, M, A)
    assert nbytes >= 256
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    n_out = max(F, 1) if n_out is None else n_out
    sse = torch.full((n_out, A, M), SENTINEL, dtype=torch.float64, device="cuda")
    wsum = torch.full((n_out,), SENTINEL, dtype=torch.float64, device="cuda")
    code = _lib.CVM_F64 if X.dtype == torch.float64 else _lib.CVM_F32
    rc = lib.cvm_pls_validation_sse(_lib.ptr(X), _lib.ptr(Y), _lib.ptr(w), _lib.ptr(idx), _lib.ptr(offsets), F, max_rows,
                                    K, M, A, code, *(_lib.ptr(s) for s in stats), _lib.ptr(B), _lib.ptr(sse),
                                    _lib.ptr(wsum), _lib.ptr(ws), nbytes - ws_short,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == want, (rc, lib.cvm_last_error())
    torch.cuda.synchronize()
    return host(sse), host(wsum)


def run(lib, d, dv=None, folds=None, **kw):
    """The design `d` (its uploaded arrays `dv`), over its own folds or over `folds`."""
    dv = upload(d) if dv is None else dv
    return score(lib, dv["X"], dv["Y"], dv["w"], d["folds"] if folds is None else folds, dv["B"], dv["stats"], **kw)


def refs_of(d, folds=None, B=None, stats=None):
    return sc.cv_reference(d["X"], d["Y"], d["w"], d["folds"] if folds is None else folds,
                           d["B"] if B is None else B, d["stats"] if stats is None else stats)


def plan(lib, F, rows, K, M, A, dtype, aligned=1):
    """cvm_cv_predict_plan with ldX = K: the scorer's plan too."""
    from cvmatrix_amd import _lib
    info = np.zeros(9, dtype=np.int64)
    code = _lib.CVM_F64 if np.dtype(dtype) == np.float64 else _lib.CVM_F32
    assert lib.cvm_cv_predict_plan(F, rows, K, K, M, A, code, aligned, ctypes.c_void_p(info.ctypes.data)) == _lib.CVM_OK
    return dict(zip(("nt", "groups", "chunks", "total", "launches", "largest", "lds", "st_in_lds", "vec"), map(int, info)))


# ------------------------------------------------------------------------------------------ (a) shape grid
def grid_cases(lib, dtype, K):
    """Folds of 1, 63, 0, 64, 65 and 129 rows (7 more rows in no fold), weights, every statistic, every (A, M) of
    predict_cases' grid: (label, sse, wsum, refs) per (A, M)."""
    rng = np.random.default_rng(13 * K + (dtype == "float32"))
    for A, M in pc.GRID_AM[dtype]:
        d = sc.design(rng, sc.SIZES, K, A, M, DT[dtype], extra=7)
        sse, wsum = run(lib, d)
        yield f"{dtype} K = {K} A = {A} M = {M}", sse, wsum, refs_of(d)


@pytest.mark.parametrize("K", pc.GRID_K)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_shape_grid(lib, dtype, K):
    worst = max(sc.assert_gate(sse, wsum, refs, what) for what, sse, wsum, refs in grid_cases(lib, dtype, K))
    print(f"test_shape_grid {dtype} K = {K}: at most {worst:.4f} of the gate")


# ------------------------------------------------------------------------------------------ (b) every variant
def variant_builds(dtype):
    f32 = dtype == "float32"
    return [(1, 4, (20, 520), (5, 25, 45, 62, 77) + ((95,) if f32 else ())),
            (0, 3, (21, 521), (7, 33, 60, 83) + ((103, 127) if f32 else ()))]


def variant_cases(lib, dtype):
    """The builds of test_gpu_pls.py::test_validation_sse_reaches_every_variant through pls_validation_sse on a
    CVMatrix that aliases the uploaded arrays (copy=False: no padding): (label, sse, wsum, refs) per (K, M, A).
    The coefficients of A models are the first A of the widest call's -- a column's reference does not depend on
    its neighbours -- so one reference per (K, M) serves every A."""
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import pls_validation_sse
    for vec, M, Ks, As in variant_builds(dtype):
        for K in Ks:
            rng = np.random.default_rng(1000 * K + M)
            d = sc.design(rng, RAGGED, K, max(As), M, DT[dtype])
            dv = upload(d)
            cvm = amd.CVMatrix(True, True, True, True, dtype=DT[dtype], copy=False)
            cvm.fit(dv["X"], dv["Y"], dv["w"])
            assert pc.same_bits(host(cvm.X), d["X"]) and pc.same_bits(host(cvm.Y), d["Y"])
            assert pc.same_bits(host(cvm.weights).reshape(-1), d["w"])
            batch = cvm.prepare_folds(d["folds"])
            full = refs_of(d)
            for A in As:
                sse, wsum = pls_validation_sse(cvm, batch, dv["stats"], dv["B"][:, :A].contiguous())
                yield f"{dtype} K = {K} M = {M} A = {A}", host(sse), host(wsum), (full[0][:, :A], full[1][:, :A], full[2], full[3])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_variant_and_both_places_of_the_statistics(lib, dtype):
    """Every instantiation of the kernel and both places of the fold's statistics against the gate.  The plan is
    asked first: the builds must reach every (column tiles, 16-byte loads) pair that exists for the element type
    and both places of the statistics, so a change of the rule cannot leave a variant untested unnoticed."""
    f32 = dtype == "float32"
    reached, places = set(), set()
    for vec, M, Ks, As in variant_builds(dtype):
        for K in Ks:
            for A in As:
                p = plan(lib, len(RAGGED), max(RAGGED), K, M, A, DT[dtype])
                assert p["vec"] == vec, (K, M, A)
                reached.add((p["nt"], vec))
                places.add(p["st_in_lds"])
    exist = {(nt, 1) for nt in range(1, 7 if f32 else 6)} | {(nt, 0) for nt in range(1, 7 if f32 else 5)}
    assert reached == exist and places == {0, 1}, (sorted(reached), sorted(places))
    worst = max(sc.assert_gate(sse, wsum, refs, what) for what, sse, wsum, refs in variant_cases(lib, dtype))
    print(f"test_every_variant_and_both_places_of_the_statistics {dtype}: at most {worst:.4f} of the gate")


# ------------------------------------------------------------------------------------------ (c) absent statistics
@pytest.mark.parametrize("K,M", [(17, 3), (16, 4)], ids=["scalar", "vector"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_combination_of_statistics_and_weights(lib, dtype, K, M):
    """NULL pointers through the C ABI for each of muX, sdX, muY, sdY and w."""
    assert plan(lib, 3, 70, K, M, 3, DT[dtype])["vec"] == (K == 16)
    rng = np.random.default_rng(23 + K)
    worst = 0.0
    for weighted in (False, True):
        for mask in itertools.product((False, True), repeat=4):
            d = sc.design(rng, (5, 0, 70), K, 3, M, DT[dtype], mask, weighted)
            sse, wsum = run(lib, d)
            worst = max(worst, sc.assert_gate(sse, wsum, refs_of(d), f"{dtype} K = {K} statistics {mask} weights {weighted}",
                                              weighted=weighted))
    print(f"test_every_combination_of_statistics_and_weights {dtype} K = {K}: at most {worst:.4f} of the gate")


# ------------------------------------------------------------------------------------------ (d) hard values
@pytest.mark.parametrize("K,A,M", [(33, 4, 5), (36, 6, 4)], ids=["scalar", "vector"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_hard_values(lib, dtype, K, A, M):
    """Columns at 1e3 times their spread, errors a thousandth of the predictions they are the difference of, muY
    1e4 times the residual, a fifth of the weights zero (sse_cases.hard_design)."""
    d = sc.hard_design(np.random.default_rng(31 + K), sc.SIZES, K, A, M, DT[dtype])
    sse, wsum = run(lib, d)
    sc.assert_gate(sse, wsum, refs_of(d), f"test_hard_values {dtype} K = {K}")


# ------------------------------------------------------------------------------------------ (e) the bit contract
@pytest.fixture(scope="module", params=[("float64", 20), ("float64", 520), ("float32", 36), ("float32", 520)],
                ids=lambda p: f"{p[0]}-K{p[1]}")
def base(lib, request):
    """One batch of ragged folds (7 rows in no fold, A = 5, M = 4: 16-byte loads), uploaded once, and its clean
    result; K = 20 / 36 keep the statistics in LDS, K = 520 reads them into registers."""
    dtype, K = request.param
    d = sc.design(np.random.default_rng(41 + K), RAGGED, K, 5, 4, DT[dtype], extra=7)
    dv = upload(d)
    p = plan(lib, len(RAGGED), max(RAGGED), K, 4, 5, DT[dtype])
    assert p["vec"] == 1 and p["st_in_lds"] == (K < 512)
    sse, wsum = run(lib, d, dv)
    sc.assert_gate(sse, wsum, refs_of(d), f"the batch of the bit tests {dtype} K = {K}")
    return dict(d=d, dv=dv, sse=sse, wsum=wsum, dtype=dtype, K=K, plan=p)


def same(got, b, folds=None):
    sse, wsum = got
    sel = slice(None) if folds is None else folds
    return pc.same_bits(sse, b["sse"][sel]) and pc.same_bits(wsum, b["wsum"][sel])


def test_a_folds_bits_depend_on_the_fold_alone(lib, base):
    """The same bits in a second call, from a workspace that held other garbage, with the fold alone, with the
    folds in reversed order, beside a 1000-row fold (16 row chunks per fold instead of 3), with max_fold_rows
    given as an upper bound, and on another stream."""
    b, d, dv = base, base["d"], base["dv"]
    F = len(d["folds"])
    assert same(run(lib, d, dv), b)
    assert same(run(lib, d, dv, ws_fill=0x42), b)                       # (finite garbage: 4.8e11 in every double)
    for f in range(F):
        one = dict(dv, B=dv["B"][f:f + 1].contiguous(), stats=tuple(s[f:f + 1].contiguous() for s in dv["stats"]))
        assert same(run(lib, d, one, folds=d["folds"][f:f + 1]), b, slice(f, f + 1)), f
    rev = dict(dv, B=dv["B"].flip(0).contiguous(), stats=tuple(s.flip(0).contiguous() for s in dv["stats"]))
    sse, wsum = run(lib, d, rev, folds=d["folds"][::-1])
    assert same((np.ascontiguousarray(sse[::-1]), np.ascontiguousarray(wsum[::-1])), b)
    # a long fold in front (rows drawn with repetition, the model of fold 0): more chunks per fold for all
    rng = np.random.default_rng(5)
    long_fold = rng.integers(0, d["X"].shape[0], 1000).astype(np.int64)
    more = dict(dv, B=torch.cat([dv["B"][:1], dv["B"]]).contiguous(), stats=tuple(torch.cat([s[:1], s]).contiguous() for s in dv["stats"]))
    sse, wsum = run(lib, d, more, folds=[long_fold] + list(d["folds"]))
    assert np.isfinite(sse[0]).all() and same((np.ascontiguousarray(sse[1:]), np.ascontiguousarray(wsum[1:])), b)
    assert same(run(lib, d, dv, max_rows=16384), b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run(lib, d, dv)
    assert same(got, b)


def test_a_prefix_of_the_models(lib, base):
    """A' < A models give the bits of sse[:, :A'] -- where the plan keeps the statistics in the same place."""
    b, d, dv = base, base["d"], base["dv"]
    for An in (1, 2):
        assert plan(lib, len(RAGGED), max(RAGGED), b["K"], 4, An, DT[b["dtype"]])["st_in_lds"] == b["plan"]["st_in_lds"]
        sse, wsum = run(lib, d, dict(dv, B=dv["B"][:, :An].contiguous()))
        assert pc.same_bits(sse, np.ascontiguousarray(b["sse"][:, :An])) and pc.same_bits(wsum, b["wsum"])


def test_alignment_does_not_matter(lib, base):
    """X, B, muX and sdX each one element into a larger buffer: the scalar-load variant, the same bits -- where
    the plan keeps the statistics in the same place."""
    b, d, dv = base, base["d"], base["dv"]
    p = plan(lib, len(RAGGED), max(RAGGED), b["K"], 4, 5, DT[b["dtype"]], aligned=0)
    assert p["vec"] == 0 and p["st_in_lds"] == b["plan"]["st_in_lds"]

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    muX, sdX, muY, sdY = dv["stats"]
    off = dict(dv, X=shifted(dv["X"]), B=shifted(dv["B"]), stats=(shifted(muX), shifted(sdX), muY, sdY))
    assert same(run(lib, d, off), b)
    for name in ("X", "B"):                                             # (one misaligned array is enough)
        assert same(run(lib, d, dict(dv, **{name: off[name]})), b), name


def test_a_row_in_two_folds(lib, base):
    """Each fold has the bits it has when the other is absent."""
    b, d, dv = base, base["d"], base["dv"]
    folds = [v.copy() for v in d["folds"]]
    folds[1] = np.concatenate([folds[1], folds[2][:1]])
    sse, wsum = run(lib, d, dv, folds=folds)
    keep = [0, 2, 3, 4]
    assert pc.same_bits(sse[keep], b["sse"][keep]) and pc.same_bits(wsum[keep], b["wsum"][keep])
    one = dict(dv, B=dv["B"][1:2].contiguous(), stats=tuple(s[1:2].contiguous() for s in dv["stats"]))
    alone = run(lib, d, one, folds=folds[1:2])
    assert pc.same_bits(alone[0], sse[1:2]) and pc.same_bits(alone[1], wsum[1:2])
    sc.assert_gate(sse, wsum, refs_of(d, folds), f"a row in two folds {b['dtype']} K = {b['K']}")


# ------------------------------------------------------------------------------------------ (f) zero and empty
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_zero_weights_and_empty_folds(lib, dtype):
    from cvmatrix_amd.pls import cv_rmse
    rng = np.random.default_rng(51)
    sizes = (5, 0, 70, 66, 0)
    d = sc.design(rng, sizes, 6, 2, 3, DT[dtype])
    d["w"][d["folds"][3]] = 0.0                                         # a fold whose weights are all zero
    dv = upload(d)
    sse, wsum = run(lib, d, dv)
    refs = refs_of(d)
    sc.assert_gate(sse, wsum, refs, f"test_zero_weights_and_empty_folds {dtype}")
    for f in (1, 3, 4):
        assert pc.same_bits(sse[f], np.zeros((2, 3))) and pc.same_bits(wsum[f:f + 1], np.zeros(1)), f
    # cv_rmse over the batch: sum over the folds, one division, one square root in float64 on top of the gate
    rmse = host(cv_rmse(torch.from_numpy(sse).cuda(), torch.from_numpy(wsum).cuda()))
    want = np.sqrt(refs[0].sum(axis=0) / refs[2].sum())
    tol = want * (refs[1].sum(axis=0) / refs[0].sum(axis=0) + refs[3].sum() / refs[2].sum() + (len(sizes) + 4) * sc.U64)
    assert rmse.shape == (2, 3) and np.isfinite(rmse).all() and (np.abs(rmse.astype(pc.LD) - want) <= tol).all()
    # every fold empty: zeros for the folds there are, nothing for the ones there are not
    none = [np.zeros(0, dtype=np.int64)] * 3
    sse, wsum = run(lib, d, dv, folds=none, n_out=5)
    assert pc.same_bits(sse[:3], np.zeros((3, 2, 3))) and pc.same_bits(wsum[:3], np.zeros(3))
    assert untouched(sse[3:]) and untouched(wsum[3:])
    sse, wsum = run(lib, d, dv, folds=[], n_out=5)                      # n_folds = 0
    assert untouched(sse) and untouched(wsum)


# ------------------------------------------------------------------------------------------ (g) limits
def one_row_folds(F, K=4):
    rng = np.random.default_rng(61)
    d = sc.design(rng, (F,), K, 1, 1, np.float64)
    perm = d["folds"][0]
    X, B, stats = pc.design(rng, F, K, 1, 1, np.float64, F=F)
    d.update(X=X, B=B, stats=stats, folds=list(perm.reshape(F, 1)))
    return d, perm


def test_the_most_folds_one_call_takes(lib):
    """F = 65535 folds of one row each (K = 4, A = M = 1): every fold against the one-row reference and gate."""
    F = 65535
    d, perm = one_row_folds(F)
    sse, wsum = run(lib, d)
    refs = sc.one_row_fold_reference(d["X"][perm], d["Y"][perm, 0], d["w"][perm], d["B"], d["stats"])
    sc.assert_gate(sse, wsum, refs, "65535 folds of one row")


def test_one_fold_too_many_is_refused(lib):
    from cvmatrix_amd import _lib
    F = 65536
    d, perm = one_row_folds(F)
    sse, wsum = run(lib, d, want=_lib.CVM_EINVAL)
    assert b"65535" in lib.cvm_last_error() and untouched(sse) and untouched(wsum)
    # the same through Python: an error, not numbers
    import cvmatrix_amd as amd
    from cvmatrix_amd.pls import pls_validation_sse
    dv = upload(d)
    cvm = amd.CVMatrix(True, True, True, True, dtype=np.float64, copy=False)
    cvm.fit(dv["X"], dv["Y"], dv["w"])
    with pytest.raises(RuntimeError, match="65535"):
        pls_validation_sse(cvm, d["folds"], dv["stats"], dv["B"])
    # (one fold fewer is fine there too)
    got = pls_validation_sse(cvm, d["folds"][:-1], tuple(s[:-1] for s in dv["stats"]), dv["B"][:-1])
    assert got[0].shape == (F - 1, 1, 1) and bool(torch.isfinite(got[0]).all())


def test_a_short_workspace_is_refused(lib):
    from cvmatrix_amd import _lib
    d = sc.design(np.random.default_rng(62), (5, 70), 6, 2, 3, np.float64)
    sse, wsum = run(lib, d, ws_short=1, want=_lib.CVM_EWORKSPACE)
    assert b"workspace" in lib.cvm_last_error() and untouched(sse) and untouched(wsum)


# ------------------------------------------------------------------------------------------ (h) non-finite values
@pytest.fixture(scope="module", params=[("float64", 20), ("float64", 520), ("float32", 20), ("float32", 520)],
                ids=lambda p: f"{p[0]}-K{p[1]}")
def three(lib, request):
    """Three folds (A = 3, M = 4) and their clean result; K = 20: statistics in LDS, K = 520: in registers."""
    dtype, K = request.param
    d = sc.design(np.random.default_rng(71 + K), (70, 65, 9), K, 3, 4, DT[dtype])
    assert plan(lib, 3, 70, K, 4, 3, DT[dtype])["st_in_lds"] == (K == 20)
    sse, wsum = run(lib, d)
    assert np.isfinite(sse).all()
    return dict(d=d, sse=sse, wsum=wsum, K=K)


def changed(d, **arrays):
    out = dict(d)
    out.update(arrays)
    return out


@pytest.mark.parametrize("what,value", [("sdX", 0.0), ("sdX", np.inf), ("sdX", -np.inf), ("sdX", np.nan), ("muX", np.inf), ("muX", np.nan)])
def test_statistics_that_are_not_finite_make_the_fold_non_finite(lib, three, what, value):
    """On both routes: never a finite number that silently ignores the column; the other folds keep their bits."""
    t, d = three, three["d"]
    i = ("muX", "sdX").index(what)
    for k in (3, t["K"] - 3):
        stats = [s.copy() for s in d["stats"]]
        stats[i][1, k] = value
        sse, wsum = run(lib, changed(d, stats=tuple(stats)))
        assert not np.isfinite(sse[1]).any(), (k, sse[1])
        assert pc.same_bits(sse[[0, 2]], t["sse"][[0, 2]]) and pc.same_bits(wsum, t["wsum"]), k


def test_a_nan_in_b_or_y_stays_in_its_column(lib, three):
    t, d = three, three["d"]
    a, m = 1, 2
    for k in (0, t["K"] - 1):
        B = d["B"].copy()
        B[1, a, k, m] = np.nan
        sse, wsum = run(lib, changed(d, B=B))
        assert np.isnan(sse[1, a, m])
        sse[1, a, m] = t["sse"][1, a, m]
        assert pc.same_bits(sse, t["sse"]) and pc.same_bits(wsum, t["wsum"]), k
    for i in (0, 64):                                                   # (a row of the fold's first and of its second chunk)
        Y = d["Y"].copy()
        Y[d["folds"][1][i], m] = np.nan
        sse, wsum = run(lib, changed(d, Y=Y))
        assert np.isnan(sse[1, :, m]).all()
        sse[1, :, m] = t["sse"][1, :, m]
        assert pc.same_bits(sse, t["sse"]) and pc.same_bits(wsum, t["wsum"]), i
