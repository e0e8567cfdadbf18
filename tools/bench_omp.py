"""Device orthogonal matching pursuit (cvm_omp_fit) timing at the C3 consumer shape (F = 10, K = 512, M = 16, A = 20)
and at F = 100, and one K = 2048, A = 64 line: device-event medians, and the same paths by scikit-learn's
orthogonal_mp_gram on the host of the same box, one thread, timed on a few (fold, response) paths and scaled to
the batch.  Nothing is gated: there is no earlier implementation and no target.

    python tools/bench_omp.py [out.txt]      (default profiles/omp/bench_omp.txt)

Designs: 4 K training rows per fold (2 K at K = 2048), unit-variance independent columns, A true nonzeros per
response, noise of the signal's size."""
import os, sys, time, warnings
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.omp import omp_fit_batched


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def make(F, K, M, n, A):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    XTX = torch.empty((F, K, K), dtype=torch.float64, device="cuda")
    XTY = torch.empty((F, K, M), dtype=torch.float64, device="cuda")
    for f in range(F):                      # (fold by fold: the rows of all folds at once need not fit)
        X = torch.randn((n, K), dtype=torch.float64, device="cuda", generator=g)
        X = X - X.mean(dim=0, keepdim=True)
        beta = torch.zeros((K, M), dtype=torch.float64, device="cuda")
        for m in range(M):
            where = torch.randperm(K, generator=g, device="cuda")[:A]
            beta[where, m] = torch.randn((A,), dtype=torch.float64, device="cuda", generator=g)
        Y = X @ beta
        Y = Y + Y.std() * torch.randn(Y.shape, dtype=torch.float64, device="cuda", generator=g)
        XTX[f], XTY[f] = X.T @ X, X.T @ (Y - Y.mean(dim=0, keepdim=True))
    return XTX, XTY


def run(name, F, K, M, A, n, out, reps=5, host_paths=3):
    XTX, XTY = make(F, K, M, n, A)
    fit = omp_fit_batched(XTX, XTY, A)
    torch.cuda.synchronize()
    ms, lo, hi = timed(lambda: omp_fit_batched(XTX, XTY, A), reps)
    n_fit = fit.n_fit.cpu().numpy()
    P = F * M
    line = (f"{name:14s} F={F:4d} K={K} M={M} A={A}: {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  "
            f"{P / ms * 1e3:8.0f} paths/s, {ms / P * 1e3:7.1f} us per path in flight with {min(P, 1024)} others   "
            f"n_fit min {n_fit.min()} max {n_fit.max()}")
    try:
        from sklearn.linear_model import orthogonal_mp_gram
        from threadpoolctl import threadpool_limits
        Gh, Hh = XTX[0].cpu().numpy(), XTY[0].cpu().numpy()
        same = True
        with warnings.catch_warnings(), threadpool_limits(1):
            warnings.simplefilter("ignore")
            orthogonal_mp_gram(Gh, Hh[:, 0], n_nonzero_coefs=A)          # (its first call pays for imports)
            t0 = time.perf_counter()
            for m in range(host_paths):
                coef = orthogonal_mp_gram(Gh, Hh[:, m], n_nonzero_coefs=A)
                same &= np.array_equal(np.flatnonzero(coef), np.sort(fit.support[0, :, m].cpu().numpy()))
        per_path = (time.perf_counter() - t0) / host_paths * 1e3
        line += (f"   scikit-learn orthogonal_mp_gram (one host thread): {per_path:8.3f} ms/path = {per_path * P:9.1f} ms "
                 f"for the batch ({per_path * P / ms:6.1f} x); the same supports: {same}")
    except ImportError:
        line += "   scikit-learn not importable: no host comparison"
    print(line, flush=True)
    out.write(line + "\n")


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "omp", "bench_omp.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as out:
        out.write(f"tools/bench_omp.py on {torch.cuda.get_device_name(0)}; device-event medians\n")
        run("C3 consumer", 10, 512, 16, 20, 2048, out)
        run("C3, 100 folds", 100, 512, 16, 20, 2048, out, reps=3)
        run("wide, all lanes", 10, 2048, 16, 64, 4096, out, reps=3)
