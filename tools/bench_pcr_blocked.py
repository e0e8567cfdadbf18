"""Blocked device PCR (cvm_pcr_blocked_fit, solver="blocked") timing, with the ROCm solver library
(torch.linalg.eigh on the same stack plus the same coefficient formula in torch operations) in the same process
and, where K <= 512, the scalar solver (cvm_pcr_fit) in the same run.  The candidates alternate inside every
repetition; each time is the median of device-event timings over the repetitions, after a warm-up call of every
candidate at the shape.  The blocked entry waits for the device once per sweep, so its time includes those waits
(the events bracket the whole call).  Sweeps and the three backward figures of tests/pcr_cases.py (residual /
||G||_F, orthogonality / sqrt(A), eigenvalue error / ||G||_F, each to be held to 60 K u), the largest over the
folds, are computed on the device.  Writes profiles/pcr/bench_pcr_blocked.txt."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvmatrix_amd.pcr import MAX_K, pcr_fit_batched

SHAPES = ((10, 512, 16, 20), (64, 1024, 32, 20), (20, 4096, 1, 20), (1000, 32, 4, 8))      # (F, K, M, A)
U = 2.0 ** -53


def timed_alternating(fns, reps):
    """Median device-event time in ms of every callable, the callables alternating inside each repetition."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in ts]


def backward(XTX, fit, lam_ref):
    A = fit.eigenvalues.shape[1]
    V, lam = fit.components, fit.eigenvalues
    nG = torch.linalg.matrix_norm(XTX)
    res = torch.linalg.matrix_norm(XTX @ V - V * lam.unsqueeze(1)) / nG
    orth = torch.linalg.matrix_norm(V.transpose(1, 2) @ V - torch.eye(A, dtype=V.dtype, device=V.device)) / A ** 0.5
    eig = (lam - lam_ref).abs().amax(dim=1) / nG
    return float(res.max()), float(orth.max()), float(eig.max())


def run(F, K, M, A, reps):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    XTX = torch.empty((F, K, K), dtype=torch.float64, device="cuda")
    XTY = torch.empty((F, K, M), dtype=torch.float64, device="cuda")
    for f in range(F):                                 # (fold by fold: X of all folds at K = 4096 is 5 GB)
        X = torch.randn((2 * K + 3, K), dtype=torch.float64, device="cuda", generator=g)
        G = X.T @ X
        XTX[f] = 0.5 * (G + G.T)
        XTY[f] = X.T @ torch.randn((2 * K + 3, M), dtype=torch.float64, device="cuda", generator=g)
    del X, G

    def blocked():
        return pcr_fit_batched(XTX, XTY, A, return_components=True, solver="blocked")

    def scalar():
        return pcr_fit_batched(XTX, XTY, A, return_components=True)

    def lib_pcr():
        lam, V = torch.linalg.eigh(XTX)
        lam, V = lam.flip(-1)[:, :A], V.flip(-1)[:, :, :A]
        T = (V.transpose(1, 2) @ XTY) / lam.unsqueeze(-1)                       # (F, A, M)
        return torch.cumsum(V.transpose(1, 2).unsqueeze(-1) * T.unsqueeze(2), dim=1), lam  # (F, A, K, M)

    fns = [blocked, lib_pcr] + ([scalar] if K <= MAX_K else [])
    fit = blocked()
    ref, lam_ref = lib_pcr()
    if K <= MAX_K:
        sfit = scalar()
    torch.cuda.synchronize()
    ms = timed_alternating(fns, reps)
    sweeps = fit.sweeps.cpu().numpy()
    res, orth, eig = backward(XTX, fit, lam_ref)
    diff = float(((fit.B - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
    line = (f"F={F:4d} K={K:4d} M={M:3d} A={A:3d}: blocked {ms[0]:10.3f} ms  sweeps {sweeps.min()}..{sweeps.max()}  "
            f"residual {res:.1e} orthogonality {orth:.1e} eigenvalues {eig:.1e} against 60 K u = {60 * K * U:.1e}   "
            f"solver library {ms[1]:10.3f} ms ({ms[1] / ms[0]:6.2f} x the blocked time), max normwise diff of B {diff:.1e}")
    if K <= MAX_K:
        ssw = sfit.sweeps.cpu().numpy()
        sdiff = float(((fit.B - sfit.B).flatten(2).norm(dim=2) / sfit.B.flatten(2).norm(dim=2)).max())
        line += (f"   scalar {ms[2]:10.3f} ms ({ms[2] / ms[0]:6.2f} x the blocked time), sweeps {ssw.min()}..{ssw.max()}, "
                 f"max normwise diff of B {sdiff:.1e}")
    print(line, flush=True)
    return line


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_pcr_blocked.py needs the GPU: a timing anywhere else says nothing.")
    out = os.path.join(ROOT, "profiles", "pcr", "bench_pcr_blocked.txt")
    lines = [f"tools/bench_pcr_blocked.py on {torch.cuda.get_device_name(0)}: median of device-event timings, "
             "the candidates alternating, one warm-up call each"]
    for F, K, M, A in SHAPES:
        lines.append(run(F, K, M, A, reps=3 if K >= 512 else 7))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
