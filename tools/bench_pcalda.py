"""Device PCA-LDA timing at the consumer shapes the other fitters use (float64): F = 10, K = 512, C = 16, A = 20 with
the scalar eigensolver, and F = 10, K = 2048, C = 16, A = 64 with the blocked one.  Device-event medians after
warm-up of
  * cvm_pcalda_fit alone (pcalda_from_components on eigenpairs that are already there) and pcalda_fit_batched
    whole, so that the eigensolve's share is visible;
  * a torch route on the device that computes the same models: torch.linalg.eigh, then per number of components
    a torch.linalg.cholesky_ex and torch.cholesky_solve on the leading block of the scores' scatter;
  * scikit-learn's Pipeline(PCA(a), LinearDiscriminantAnalysis(solver="lsqr")) refitted on the training rows, on
    the host of the same box, timed on fold 0 with two numbers of components and scaled to the F A fits.
Nothing is gated: there is no earlier implementation and no target.

    python tools/bench_pcalda.py [out.txt]      (default profiles/pcalda/bench_pcalda.txt)
    python tools/bench_pcalda.py --kernels-only (three calls of cvm_pcalda_fit per shape and nothing else: the
                                                 program to run under a kernel trace for the expand kernel's rate)

Designs: 4 K training rows per fold (2 K at K = 2048), latent standard deviations 0.98^k mixed by a rotation, class
means of that size, classes of unequal size."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd.pcalda import pcalda_fit_batched, pcalda_from_components
from cvmatrix_amd.pcr import pcr_fit_batched

SHAPES = (("C3 consumer", 10, 512, 16, 20, 2048, "scalar", 5), ("C3 consumer", 10, 512, 16, 20, 2048, "blocked", 5),
          ("wide", 10, 2048, 16, 64, 4096, "blocked", 3))


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
    s = 0.98 ** torch.arange(K, dtype=torch.float64, device="cuda")
    mix = torch.linalg.qr(torch.randn((K, K), dtype=torch.float64, device="cuda", generator=g))[0]
    rows0 = None
    for f in range(F):                      # (fold by fold: the rows of all folds at once need not fit)
        means = 1.5 * torch.randn((C, K), dtype=torch.float64, device="cuda", generator=g) * s
        X = (torch.randn((n, K), dtype=torch.float64, device="cuda", generator=g) * s + means[y]) @ mix
        X = X - X.mean(dim=0, keepdim=True)
        XTX[f], XTY[f], CW[f] = X.T @ X, X.T @ Y, Y.sum(dim=0)
        if f == 0:
            rows0 = (X.cpu().numpy(), y.cpu().numpy())
    return XTX, XTY, CW, rows0


def torch_route(XTX, XTY, CW, A):
    """coef (F, A, K, C), intercept (F, A, C) by torch operations alone."""
    F, K, C = XTY.shape
    lam, Q = torch.linalg.eigh(XTX)
    lam, V = lam.flip(1)[:, :A], Q.flip(2)[:, :, :A]
    P = V.transpose(1, 2) @ XTY
    Mt = P / CW[:, None, :]
    S = torch.diag_embed(lam) - Mt @ P.transpose(1, 2)
    n = CW.sum(dim=1)
    coef = torch.empty((F, A, K, C), dtype=XTX.dtype, device=XTX.device)
    icpt = torch.empty((F, A, C), dtype=XTX.dtype, device=XTX.device)
    prior = torch.log(CW / n[:, None])
    for a in range(A):
        Lc, _ = torch.linalg.cholesky_ex(S[:, :a + 1, :a + 1])
        x = torch.cholesky_solve(Mt[:, :a + 1], Lc)
        coef[:, a] = n[:, None, None] * (V[:, :, :a + 1] @ x)
        icpt[:, a] = -0.5 * n[:, None] * (Mt[:, :a + 1] * x).sum(dim=1) + prior
    return coef, icpt


def run(name, F, K, C, A, n, solver, reps, out):
    XTX, XTY, CW, (X0, y0) = make(F, K, C, n)
    fit = pcalda_fit_batched(XTX, XTY, CW, A, solver=solver, check=True)
    pca = pcr_fit_batched(XTX, None, A, return_components=True, solver=solver)
    ref_coef, ref_icpt = torch_route(XTX, XTY, CW, A)
    torch.cuda.synchronize()
    # (the two routes hold different eigenvectors of the same matrix: their models agree to the subspaces' accuracy)
    ok = torch.isfinite(ref_coef).flatten(1).all(dim=1)                # (folds where the torch route itself stayed finite)
    diff = float(((fit.coef[ok] - ref_coef[ok]).norm() / ref_coef[ok].norm()).item()) if bool(ok.any()) else float("nan")
    lost = int((~ok).sum().item())
    own = lambda: pcalda_from_components(pca.components, pca.eigenvalues, pca.n_fit, XTY, CW)      # noqa: E731
    own()
    ms, lo, hi = timed(own, reps + 4)
    wms, wlo, whi = timed(lambda: pcalda_fit_batched(XTX, XTY, CW, A, solver=solver), reps)
    tms, tlo, thi = timed(lambda: torch_route(XTX, XTY, CW, A), reps)
    stored = F * A * K * C * 8
    line = (f"{name:12s} F={F} K={K} C={C} A={A}: cvm_pcalda_fit alone {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}; coef is "
            f"{stored / 1e6:.1f} MB), pcalda_fit_batched whole ({solver} eigensolver) {wms:9.3f} ms (min {wlo:.3f}, max "
            f"{whi:.3f}; {reps} runs): the eigensolve is {100 * (1 - ms / wms):.3f} % of it;  torch route (eigh, then "
            f"cholesky_ex + cholesky_solve per a) {tms:9.3f} ms (min {tlo:.3f}, max {thi:.3f}) = {tms / wms:6.3f} x the "
            f"whole;  n_fit {fit.n_fit.cpu().tolist()};  coef against the torch route {diff:.1e} relative"
            + (f" ({lost} fold(s) left out: the torch route is not finite there)" if lost else ""))
    try:
        from sklearn.decomposition import PCA
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
        from sklearn.pipeline import make_pipeline
        make_pipeline(PCA(2, svd_solver="full"), LinearDiscriminantAnalysis(solver="lsqr")).fit(X0[:8 * C], y0[:8 * C])
        t0 = time.perf_counter()
        for a in (max(1, A // 4), A):
            make_pipeline(PCA(a, svd_solver="full"), LinearDiscriminantAnalysis(solver="lsqr")).fit(X0, y0)
        per_fit = (time.perf_counter() - t0) / 2 * 1e3
        line += (f";  scikit-learn Pipeline(PCA, LDA lsqr) refit on {n} rows (host, its own threads): {per_fit:9.1f} ms/fit "
                 f"= {per_fit * F * A:10.1f} ms for the batch ({per_fit * F * A / wms:7.1f} x)")
    except ImportError:
        line += ";  scikit-learn not importable: no host comparison"
    print(line, flush=True)
    out.write(line + "\n")


def kernels_only():
    for name, F, K, C, A, n, solver, _ in SHAPES:
        XTX, XTY, CW, _ = make(F, K, C, n)
        pca = pcr_fit_batched(XTX, None, A, return_components=True, solver=solver)
        for _ in range(3):
            pcalda_from_components(pca.components, pca.eigenvalues, pca.n_fit, XTY, CW)
        torch.cuda.synchronize()
        print(f"{name}: F={F} K={K} C={C} A={A}: coef {F * A * K * C * 8} bytes per call", flush=True)


if __name__ == "__main__":
    if "--kernels-only" in sys.argv:
        kernels_only()
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "pcalda", "bench_pcalda.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as out:
        out.write(f"tools/bench_pcalda.py on {torch.cuda.get_device_name(0)}; device-event medians, float64\n")
        for name, F, K, C, A, n, solver, reps in SHAPES:
            run(name, F, K, C, A, n, solver, reps, out)
