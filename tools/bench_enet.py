"""Device elastic net / lasso (cvm_enet_fit) timing at the C3 consumer shape (F = 10, K = 512, M = 16, L = 20) and
at F = 100, l1_ratio 1 and 0.5, penalties lambda_grid(eps=1e-3), defaults tol = 1e-8 and max_sweeps = 1000:
device-event medians, the sweeps per problem, and the same solves by scikit-learn's Gram-precomputed
coordinate descent (enet_path with precompute=G, Xy=h: warm starts down the same grid) on the host of the same
box, timed on a few (fold, response) paths and scaled to the batch.

    python tools/bench_enet.py [out.txt]      (default profiles/enet/bench_enet.txt)

Designs: 4 K training rows per fold, unit-variance columns, 16 true nonzeros per response, noise of the signal's
size; once with independent columns (cond(XTX) about 9) and once with a shared factor (pairwise correlation 0.2,
cond(XTX) about 500: coordinate descent then needs thousands of sweeps for the dense end of the grid)."""
import os, sys, time, warnings
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.enet import enet_fit_batched, lambda_grid


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def make(F, K, M, n, corr):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    X = torch.randn((F, n, K), dtype=torch.float64, device="cuda", generator=g)
    X = np.sqrt(1 - corr) * X + np.sqrt(corr) * torch.randn((F, n, 1), dtype=torch.float64, device="cuda", generator=g)
    X = X - X.mean(dim=1, keepdim=True)
    beta = torch.zeros((F, K, M), dtype=torch.float64, device="cuda")
    for m in range(M):
        where = torch.randperm(K, generator=g, device="cuda")[:16]
        beta[:, where, m] = torch.randn((F, 16), dtype=torch.float64, device="cuda", generator=g)
    Y = X @ beta
    Y = Y + Y.std() * torch.randn(Y.shape, dtype=torch.float64, device="cuda", generator=g)
    Y = Y - Y.mean(dim=1, keepdim=True)
    return X, Y, X.transpose(1, 2) @ X, X.transpose(1, 2) @ Y


def run(name, F, K, M, L, rho, corr, out, reps=5, warm=1, host_paths=3):
    n = 4 * K
    X, Y, XTX, XTY = make(F, K, M, n, corr)
    lam = lambda_grid(XTY, rho, L, 1e-3)
    for _ in range(warm):
        fit = enet_fit_batched(XTX, XTY, lam, rho)
    torch.cuda.synchronize()
    ms, lo, hi = timed(lambda: enet_fit_batched(XTX, XTY, lam, rho), reps)
    info, sweeps = fit.info.cpu().numpy(), fit.sweeps.cpu().numpy()
    nnz = (fit.B != 0).sum(dim=2).cpu().numpy()
    P = F * M * L
    line = (f"{name:14s} F={F:4d} K={K} M={M} L={L} l1_ratio={rho:3.1f} correlation={corr:3.1f}: {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  "
            f"{P / ms * 1e3:8.0f} problems/s   info 0/1/2: {(info == 0).sum()}/{(info == 1).sum()}/{(info == 2).sum()}   "
            f"sweeps per problem: mean {sweeps.mean():.1f}, median {np.median(sweeps):.0f}, max {sweeps.max()}; "
            f"per path (all {L} penalties): mean {sweeps.sum(axis=1).mean():.0f}, max {sweeps.sum(axis=1).max()}   "
            f"nonzeros at the smallest penalty: mean {nnz[:, -1].mean():.0f}, max {nnz[:, -1].max()} "
            f"(paths that left the 64-coordinate active set: {(nnz.max(axis=1) > 64).sum()} of {F * M} at least)")
    try:
        from sklearn.linear_model import enet_path
        Xh, Yh, Gh, Hh = (t[0].cpu().numpy() for t in (X, Y, XTX, XTY))
        t0 = time.perf_counter()
        worst = 0.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for m in range(host_paths):
                _, coefs, _ = enet_path(Xh, Yh[:, m], l1_ratio=rho, alphas=lam / n, precompute=Gh, Xy=Hh[:, m],
                                        tol=1e-8, max_iter=1000)
                got = fit.B[0, :, :, m].cpu().numpy().T
                worst = max(worst, float(np.abs(coefs - got).max() / np.abs(coefs).max()))
        per_path = (time.perf_counter() - t0) / host_paths * 1e3
        line += (f"   scikit-learn enet_path (Gram precomputed, tol 1e-8 on its dual gap, one host thread): {per_path:8.2f} ms/path "
                 f"= {per_path * F * M:9.1f} ms for the batch ({per_path * F * M / ms:6.1f} x); largest coefficient difference "
                 f"{worst:.1e} of the largest coefficient")
    except ImportError:
        line += "   scikit-learn not importable: no host comparison"
    print(line, flush=True)
    out.write(line + "\n")


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "enet", "bench_enet.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as out:
        out.write(f"tools/bench_enet.py on {torch.cuda.get_device_name(0)}; device-event medians\n")
        for corr in (0.0, 0.2):
            for rho in (1.0, 0.5):
                run("C3 consumer", 10, 512, 16, 20, rho, corr, out)
            for rho in (1.0, 0.5):
                run("C3, 100 folds", 100, 512, 16, 20, rho, corr, out, reps=3)
