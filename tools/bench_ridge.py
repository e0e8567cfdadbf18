"""Device ridge (cvm_ridge_fit) timing at the consumer shapes, with the ROCm solver library
(torch.linalg.cholesky_ex + torch.cholesky_solve) on the same batch in the same run as a yardstick and
NumPy on the host.  Flops per call F L (K^3/3 + 2 K^2 M); peak 78.6 TFLOP/s fp64 MFMA on 256 CUs."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.ridge import ridge_fit_batched

PEAK_TF, CUS = 78.6, 256


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run(name, F, K, M, L, dtype=torch.float64, reps=7, warm=2, yardstick=True):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    X = torch.randn((F, K + 64, K), dtype=torch.float64, device="cuda", generator=g)
    XTX = (X.transpose(1, 2) @ X).to(dtype)
    XTY = (X.transpose(1, 2) @ torch.randn((F, K + 64, M), dtype=torch.float64, device="cuda", generator=g)).to(dtype)
    del X
    tr = float(XTX.double().diagonal(dim1=1, dim2=2).sum(-1).mean()) / K
    lam = np.logspace(-4, 1, L) * tr
    for _ in range(warm):
        fit = ridge_fit_batched(XTX, XTY, lam)
    torch.cuda.synchronize()
    ms = timed(lambda: ridge_fit_batched(XTX, XTY, lam), reps)
    P = F * L
    flop = P * (K ** 3 / 3 + 2 * K * K * M)
    tf = flop / ms / 1e9
    bound_ms = flop / min(P, CUS) / (PEAK_TF * 1e12 / CUS) * 1e3 if P <= CUS else flop / (PEAK_TF * 1e12) * 1e3
    line = (f"{name:18s} F={F:4d} K={K:5d} M={M:3d} L={L:3d} {str(dtype)[6:]:8s}: {ms:9.3f} ms  {P / ms * 1e3:9.0f} problems/s  "
            f"{tf:6.2f} TFLOP/s ({tf / PEAK_TF * 100:5.1f} % of peak, {bound_ms / ms * 100:5.1f} % of the "
            f"one-workgroup-per-problem bound {bound_ms:.3f} ms)")
    # yardstick: the same batch through the ROCm solver library, float64, same timing
    lam_t = torch.from_numpy(lam).cuda()
    A64, Y64 = XTX.double(), XTY.double()
    eye = torch.eye(K, dtype=torch.float64, device="cuda")

    def lib_solve():
        A = A64.unsqueeze(1) + lam_t.view(1, L, 1, 1) * eye
        Lf, _ = torch.linalg.cholesky_ex(A)
        return torch.cholesky_solve(Y64.unsqueeze(1).expand(F, L, K, M), Lf)
    try:
        if not yardstick:
            raise RuntimeError("not run at this shape (its batched K = 4096 factorisation ended in a launch failure)")
        ref = lib_solve(); torch.cuda.synchronize()
        ms_lib = timed(lib_solve, reps)
        diff = float(((fit.B.double() - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
        line += f"   solver library {ms_lib:9.3f} ms ({ms_lib / ms:5.2f} x), max normwise diff {diff:.1e}"
        del ref
    except RuntimeError as e:                      # (out of memory at the big shapes)
        line += f"   solver library: {str(e).splitlines()[0][:60]}"
    a, b = A64[0].cpu().numpy(), Y64[0].cpu().numpy()
    t0 = time.perf_counter()
    for lv in lam[:2]:
        c = np.linalg.cholesky(a + lv * np.eye(K)); np.linalg.solve(c.T, np.linalg.solve(c, b))
    line += f"   numpy {(time.perf_counter() - t0) / 2 * 1e3:8.2f} ms/problem"
    print(line, flush=True)


if __name__ == "__main__":
    run("C3 consumer", 10, 512, 16, 20)
    run("C3, 100 folds", 100, 512, 16, 10)
    run("C4 consumer", 64, 1024, 32, 10)
    run("C5 consumer", 20, 4096, 1, 4, dtype=torch.float32, reps=3, warm=1, yardstick=False)
