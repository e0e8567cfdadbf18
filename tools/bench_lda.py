"""Device LDA (cvm_lda_fit) timing at the C3 consumer shape (F = 10, K = 512, C = 16, L = 20) and at K = 2048:
device-event medians of lda_fit_batched, of the ridge solve alone on the same shape (what is left is the two LDA
kernels), and two baselines that compute the same models:
  * a torch route on the device: the downdate as a batched matrix product, then per shrinkage
    torch.linalg.cholesky_ex and torch.cholesky_solve on the shrunk covariances of all folds;
  * scikit-learn's LinearDiscriminantAnalysis(solver="lsqr", shrinkage=g) refitted on the training rows, on the
    host of the same box, timed on fold 0 with two shrinkages and scaled to the F L fits of the batch.
Nothing is gated: there is no earlier implementation and no target.

    python tools/bench_lda.py [out.txt]      (default profiles/lda/bench_lda.txt)

Designs: 4 K training rows per fold (2 K at K = 2048), unit within-class variance, class means two standard
deviations apart, classes of unequal size; shrinkage = linspace(0, 1, L)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.lda import lda_fit_batched
from cvmatrix_amd.ridge import ridge_fit_batched


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def make(F, K, C, n):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    XTX = torch.empty((F, K, K), dtype=torch.float64, device="cuda")
    XTY = torch.empty((F, K, C), dtype=torch.float64, device="cuda")
    CW = torch.empty((F, C), dtype=torch.float64, device="cuda")
    y = (torch.arange(n, device="cuda") % (C + 1)) % C
    Y = torch.nn.functional.one_hot(y, C).to(torch.float64)
    rows0 = None
    for f in range(F):                      # (fold by fold: the rows of all folds at once need not fit)
        means = torch.randn((C, K), dtype=torch.float64, device="cuda", generator=g)
        means = 2.0 * means / means.norm(dim=1, keepdim=True)
        X = torch.randn((n, K), dtype=torch.float64, device="cuda", generator=g) + means[y]
        X = X - X.mean(dim=0, keepdim=True)
        XTX[f], XTY[f], CW[f] = X.T @ X, X.T @ Y, Y.sum(dim=0)
        if f == 0:
            rows0 = (X.cpu().numpy(), y.cpu().numpy())
    return XTX, XTY, CW, rows0


def torch_route(XTX, XTY, CW, gammas):
    """coef (F, L, K, C), intercept (F, L, C) by torch operations alone."""
    F, K, C = XTY.shape
    Mc = XTY / CW[:, None, :]
    Sw = XTX - Mc @ XTY.transpose(1, 2)
    n = CW.sum(dim=1)
    tr = torch.diagonal(Sw, dim1=1, dim2=2).sum(dim=1)
    eye = torch.eye(K, dtype=XTX.dtype, device=XTX.device)
    coef = torch.empty((F, len(gammas), K, C), dtype=XTX.dtype, device=XTX.device)
    for l, gm in enumerate(gammas):
        cov = (1.0 - gm) * Sw / n[:, None, None] + (gm * tr / (n * K))[:, None, None] * eye
        Lc, _ = torch.linalg.cholesky_ex(cov)
        coef[:, l] = torch.cholesky_solve(Mc, Lc)
    icpt = -0.5 * (Mc[:, None] * coef).sum(dim=2) + torch.log(CW / n[:, None])[:, None, :]
    return coef, icpt


def run(name, F, K, C, L, n, out, reps=5):
    XTX, XTY, CW, (X0, y0) = make(F, K, C, n)
    gammas = np.linspace(0.0, 1.0, L)
    fit = lda_fit_batched(XTX, XTY, CW, gammas, check=True)
    ref_coef, ref_icpt = torch_route(XTX, XTY, CW, gammas)
    torch.cuda.synchronize()
    diff = float(((fit.coef - ref_coef).norm() / ref_coef.norm()).item())
    ms, lo, hi = timed(lambda: lda_fit_batched(XTX, XTY, CW, gammas), reps)
    lam = gammas[:-1] / (1.0 - gammas[:-1])
    ridge_fit_batched(XTX, XTY, lam)
    rms, _, _ = timed(lambda: ridge_fit_batched(XTX, XTY, lam), reps)
    tms, tlo, thi = timed(lambda: torch_route(XTX, XTY, CW, gammas), reps)
    moved = F * 8 * (2 * K * K + (1 + 2 * L) * K * C)    # stage 1 reads XTX, writes S'; stage 3 reads x, writes coef
    line = (f"{name:12s} F={F} K={K} C={C} L={L}: lda_fit_batched {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs), "
            f"the ridge solve alone on this shape {rms:9.3f} ms, the two LDA stages by difference {ms - rms:8.3f} ms "
            f"for {moved / 1e6:.1f} MB moved;  torch route (cholesky_ex + cholesky_solve per shrinkage) {tms:9.3f} ms "
            f"(min {tlo:.3f}, max {thi:.3f}) = {tms / ms:5.2f} x;  coef against the torch route {diff:.1e} relative")
    try:
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
        LinearDiscriminantAnalysis(solver="lsqr", shrinkage=0.5).fit(X0[:4 * C], y0[:4 * C])     # (imports)
        t0 = time.perf_counter()
        for gm in (0.25, 0.75):
            LinearDiscriminantAnalysis(solver="lsqr", shrinkage=gm).fit(X0, y0)
        per_fit = (time.perf_counter() - t0) / 2 * 1e3
        line += (f";  scikit-learn lsqr refit on {n} rows (host, its own threads): {per_fit:9.1f} ms/fit = "
                 f"{per_fit * F * L:10.1f} ms for the batch ({per_fit * F * L / ms:7.1f} x)")
    except ImportError:
        line += ";  scikit-learn not importable: no host comparison"
    print(line, flush=True)
    out.write(line + "\n")


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "lda", "bench_lda.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as out:
        out.write(f"tools/bench_lda.py on {torch.cuda.get_device_name(0)}; device-event medians\n")
        run("C3 consumer", 10, 512, 16, 20, 2048, out)
        run("wide", 10, 2048, 16, 20, 4096, out, reps=3)
