"""Training matrices of unions of folds (cvm_sweep_unions through CVMatrix.training_XTX_XTY_unions) against the
only route the library had before: the same training sets as folds of concatenated index arrays, which are not a
partition and so take the general fold update (the Gram kernel over every removed row again).  Both in one
process on one device, alternating call by call; medians of device-event timings after a warm-up; the lists of
unions and folds are prepared and uploaded before the warm-up and every timed call's outputs come out of
torch's cached blocks (README "Round 6": an allocation between warm-up and timed steps is what gets timed).

    python tools/bench_unions.py            # prints; kept in profiles/unions/bench_unions.txt

Line 1: the 45 pair matrices of the C3 workload (BASELINE.json: N = 100 000, K = 512, M = 16, 10 folds,
weighted, all four flags, float64).  Line 2: float32, K = 1024, 20 folds (190 pairs): the HBM side -- bytes the
union kernels move per second (outputs written once; per output tile the G tile and one partial per fold of
the union read, counted once: the folds' partials are shared by the unions through L2 / MALL only in part)
next to the rate of cvm_fill_probe (the device's write ceiling with the same kind of store) on the very
output buffer."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvmatrix_amd import CVMatrix, Partitioner, _lib  # noqa: E402
from cvmatrix_amd.unions import fold_pairs, prepare_unions  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(name, N, K, M, P, dtype, parent=True, reps=20, warm=3):
    rng = np.random.default_rng(42)
    X = rng.random((N, K)).astype(dtype)
    Y = rng.random((N, M)).astype(dtype)
    w = (rng.random(N) + 0.1).astype(dtype)
    labels = np.arange(N) % P
    part = Partitioner(labels)
    cvm = CVMatrix(dtype=dtype)
    cvm.fit(X, Y, w, folds=part)
    batch = cvm.sweep_folds
    pairs = fold_pairs(P)
    ub = prepare_unions(pairs, P)
    es = np.dtype(dtype).itemsize
    U = len(pairs)

    def unions():
        return cvm.training_XTX_XTY_unions(batch, ub)

    fns = [unions]
    if parent:
        arrays = [part.get_validation_indices(k) for k in part.folds_dict]
        concat = cvm.prepare_folds([np.concatenate([arrays[f], arrays[g]]) for f, g in pairs])

        def general():
            return cvm.training_XTX_XTY_batched(concat)

        fns.append(general)
    for _ in range(warm):
        for fn in fns:
            res = fn()
            del res
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):                        # alternating: the clock and the neighbours are shared
        for t, fn in zip(times, fns):
            t.append(event_ms(fn))
    med = [float(np.median(t)) for t in times]
    # bytes of the union route: outputs once, G tile + one partial per fold of the pair per output element (XTX:
    # the upper triangle of tiles is read, both triangles are written)
    Kd, Md = cvm._Kd, cvm._Md or 0
    out_b = U * (Kd * Kd + Kd * Md) * es
    read_b = U * ((Kd * Kd // 2) * 3 + Kd * Md * 3) * es
    line = (f"{name:12s} N={N} K={K} M={M} folds={P} unions={U} {np.dtype(dtype).name}: unions {med[0]:8.3f} ms "
            f"({(out_b + read_b) / med[0] / 1e9:7.2f} TB/s moved, {out_b / 1e9:.3f} GB written + {read_b / 1e9:.3f} GB read)")
    if parent:
        (ax, ay), _ = unions()
        (bx, by), _ = general()
        diff = float((ax - bx).abs().max() / bx.abs().max())
        line += f"  general fold update on concatenated indices {med[1]:8.3f} ms ({med[1] / med[0]:6.1f} x), max diff {diff:.1e}"
        del ax, ay, bx, by
    else:
        (ax, ay), _ = unions()
        lib = _lib.load()
        nbytes = ax.numel() * es
        fill = [event_ms(lambda: lib.cvm_fill_probe(ax.data_ptr(), nbytes, cvm._stream())) for _ in range(reps + warm)][warm:]
        fill_ms = float(np.median(fill))
        fill_rate, rate = nbytes / fill_ms / 1e9, (out_b + read_b) / med[0] / 1e9
        line += (f"  cvm_fill_probe on the XTX output ({nbytes / 1e9:.3f} GB) {fill_ms:7.3f} ms = {fill_rate:5.2f} TB/s; "
                 f"achieved / fill rate = {rate / fill_rate:4.2f}")
    print(line, flush=True)


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), "|", _lib.load().cvm_version().decode(), flush=True)
    run("C3 pairs", 100000, 512, 16, 10, np.float64)
    run("HBM side", 100000, 1024, 16, 20, np.float32, parent=False)
