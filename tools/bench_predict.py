"""Device predictions (cvm_cv_predict through cv_predict) at the consumer shapes, with two yardsticks in the same
process: the scorer pls_validation_sse on the same inputs (it forms the same products and keeps one sum per
fold, model and response), alternating with cv_predict call by call, and the torch loop a user would write
(one gather and one batched matmul per fold).  Medians of device-event timings after a warm-up of every
shape.  The store bound of the last column: N A M elements at the plain-store rate of the chip (6.0 TB/s).
The accuracy column: the largest |out - ref| / gate of tests/predict_cases.py over a sample of rows (the
np.longdouble reference of all rows would take minutes)."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cvmatrix_amd import CVMatrix, Partitioner
from cvmatrix_amd.pls import pls_validation_sse
from cvmatrix_amd.predict import cv_predict
import predict_cases as pc


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(name, N, F, K, M, A, reps=20, warm=3):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, K)) * rng.uniform(0.5, 2.0, K) + rng.standard_normal(K)
    Y = rng.standard_normal((N, M)) + 3
    labels = np.arange(N) % F
    cvm = CVMatrix(dtype=np.float64)
    cvm.fit(X, Y)
    part = Partitioner(labels)
    batch = cvm.prepare_folds(part)
    _, stats = cvm.training_XTX_XTY_batched(batch)
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    B = torch.randn((F, A, K, M), dtype=torch.float64, device="cuda", generator=g) * 0.05
    out = torch.empty((N, A, M), dtype=torch.float64, device="cuda")
    vals = [torch.from_numpy(part.get_validation_indices(k)).cuda() for k in part.folds_dict]
    muX, sdX, muY, sdY = stats

    def predict():
        return cv_predict(cvm, batch, stats, B, out=out)

    def scorer():
        return pls_validation_sse(cvm, batch, stats, B)

    def loop():
        res = torch.empty((N, A, M), dtype=torch.float64, device="cuda")
        for f, v in enumerate(vals):
            z = (cvm.X[v] - muX[f]) / sdX[f]
            res[v] = (torch.matmul(z, B[f]) * sdY[f] + muY[f]).transpose(0, 1)      # (A, n, M) -> (n, A, M)
        return res

    for _ in range(warm):
        predict(); scorer(); ref_loop = loop()
    torch.cuda.synchronize()
    tp, ts, tl = [], [], []
    for _ in range(reps):                       # alternating: the clock and the neighbours are shared
        tp.append(event_ms(predict)); ts.append(event_ms(scorer))
    for _ in range(max(3, reps // 4)):
        tl.append(event_ms(loop))
    tp, ts, tl = float(np.median(tp)), float(np.median(ts)), float(np.median(tl))
    # accuracy on a sample of rows, against the loop as well (its own rounding: a loose look, not a gate)
    got = predict()
    loop_diff = float((got - ref_loop).abs().max() / ref_loop.abs().max())
    rows = np.unique(rng.integers(0, N, 193))
    hX, hB, hst = cvm.X[rows].cpu().numpy(), B.cpu().numpy(), tuple(s.cpu().numpy() for s in stats)
    hout = got[rows].cpu().numpy()
    worst = 0.0
    for i, r in enumerate(rows):
        f = int(labels[r])
        ref, gate = pc.reference(hX[i:i + 1], hB[f], pc.fold_stats(hst, f))
        worst = max(worst, pc.worst_ratio(hout[i:i + 1], ref, gate))
    store_ms = N * A * M * 8 / 6.0e12 * 1e3
    flops = 2.0 * N * K * A * M
    print(f"{name:14s} N={N:6d} F={F:4d} K={K:4d} M={M:3d} A={A:3d}: cv_predict {tp:8.3f} ms ({flops / tp / 1e9:6.1f} TFLOP/s)  "
          f"scorer {ts:8.3f} ms ({tp / ts:5.2f} x)  scorer + store bound {store_ms:6.3f} ms + 10 % = {(ts + store_ms) * 1.1:8.3f} ms  "
          f"torch loop {tl:8.3f} ms ({tl / tp:6.2f} x), max diff {loop_diff:.1e}  gate ratio {worst:.3f} ({rows.size} rows)",
          flush=True)


if __name__ == "__main__":
    run("C3 consumer", 100000, 10, 512, 16, 20)
    run("100 folds", 100000, 100, 128, 16, 20)
    run("1000 folds", 100000, 1000, 32, 4, 8)
