"""Device PCR (cvm_pcr_fit) timing at the consumer shapes, with the ROCm solver library (torch.linalg.eigh on
the same stack plus the same coefficient formula in torch operations) in the same run as a yardstick.
Median of device-event timings.  Cost model of the kernel: a round reads and writes S and V once, a sweep of
K - 1 rounds moves about 32 K^3 bytes per fold through one CU."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.pcr import pcr_fit_batched


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run(name, F, K, M, A, reps=5, warm=1):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    X = torch.randn((F, 2 * K + 3, K), dtype=torch.float64, device="cuda", generator=g)
    XTX = X.transpose(1, 2) @ X
    XTX = 0.5 * (XTX + XTX.transpose(1, 2))
    XTY = X.transpose(1, 2) @ torch.randn((F, 2 * K + 3, M), dtype=torch.float64, device="cuda", generator=g)
    del X
    for _ in range(warm):
        fit = pcr_fit_batched(XTX, XTY, A)
    torch.cuda.synchronize()
    ms = timed(lambda: pcr_fit_batched(XTX, XTY, A), reps)
    sweeps = fit.sweeps.cpu().numpy()
    gb = 32.0 * K ** 3 * float(sweeps.sum()) / 1e9
    line = (f"{name:14s} F={F:4d} K={K:4d} M={M:3d} A={A:3d}: {ms:10.3f} ms  {F / ms * 1e3:9.0f} folds/s  sweeps "
            f"{sweeps.min()}..{sweeps.max()}  model traffic {gb:8.2f} GB = {gb / ms:7.1f} GB/ms")

    def lib_pcr():
        lam, V = torch.linalg.eigh(XTX)
        lam, V = lam.flip(-1)[:, :A], V.flip(-1)[:, :, :A]
        T = (V.transpose(1, 2) @ XTY) / lam.unsqueeze(-1)                       # (F, A, M)
        return torch.cumsum(V.transpose(1, 2).unsqueeze(-1) * T.unsqueeze(2), dim=1)  # (F, A, K, M)
    try:
        ref = lib_pcr(); torch.cuda.synchronize()
        ms_lib = timed(lib_pcr, reps)
        diff = float(((fit.B - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
        line += f"   solver library {ms_lib:10.3f} ms ({ms_lib / ms:6.2f} x), max normwise diff {diff:.1e}"
    except RuntimeError as e:
        line += f"   solver library: {str(e).splitlines()[0][:60]}"
    print(line, flush=True)


if __name__ == "__main__":
    run("C3 consumer", 10, 512, 16, 20, reps=3)
    run("100 folds", 100, 128, 16, 20)
    run("1000 folds", 1000, 32, 4, 8)
