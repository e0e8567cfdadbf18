"""Fast cross-validation of the elastic net (or the lasso) over a grid of penalties, end to end on one MI355X.

    python examples/fast_cv_enet.py [N K M folds [l1_ratio]]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY, means, stds of every fold        (HIP)
2. lambda_grid + enet_fit_batched            coordinate descent on (XtX, XtY) for every fold, response
                                             and lambda, warm-started down the grid                    (HIP)
3. pls_validation_sse                        squared validation errors of every fold's models          (HIP)
   -> RMSE per lambda.  (Shapes whose device copies are padded -- odd K, float64 with odd M -- take the
   same formula in plain torch operations.)

Where scikit-learn is importable the RMSE of three of the penalties is checked against ElasticNet refitted on
every training set: alpha = lambda / n_train, fit_intercept=True on the raw rows (= centring with the training
means)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.enet import enet_fit_batched, lambda_grid  # noqa: E402
from cvmatrix_amd.pls import cv_rmse, pls_validation_sse  # noqa: E402


def fast_cv_rmse(X, Y, labels, l1_ratio=0.5, lambdas=None, n_lambdas=20, eps=1e-3, tol=1e-8):
    """(lambdas, RMSE[l, m], nonzeros[l, m]): RMSE over all validation rows for elastic net models with penalty
    lambdas[l] on centred X and Y (an intercept), every row predicted by the model that was trained without its
    fold; nonzeros: the mean number of nonzero coefficients over the folds.  ``lambdas`` None: ``lambda_grid``
    of the folds' own XTY.  X, Y: NumPy arrays."""
    p = Partitioner(labels)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(p)
    (XTX, XTY), (muX, sdX, muY, sdY) = cvm.training_XTX_XTY_batched(batch)
    if lambdas is None:
        lambdas = lambda_grid(XTY, l1_ratio, n_lambdas, eps)
    B = enet_fit_batched(XTX, XTY, lambdas, l1_ratio, tol=tol, check=True).B          # (F, L, K, M)
    nonzeros = (B != 0).sum(dim=2).double().mean(dim=0).cpu().numpy()
    if cvm._Kd == cvm._Ku and (cvm._Md or 0) == (cvm._Mu or 0):
        sse_f, wsum_f = pls_validation_sse(cvm, batch, (muX, sdX, muY, sdY), B)
        return np.asarray(lambdas), cv_rmse(sse_f, wsum_f).cpu().numpy(), nonzeros
    sse = torch.zeros((B.shape[1], Y.shape[1]), dtype=torch.float64, device=B.device)
    for f, key in enumerate(p.folds_dict):
        val = torch.from_numpy(p.get_validation_indices(key)).to(B.device)
        pred = torch.matmul(cvm.X[val] - muX[f], B[f]) + muY[f]         # (L, n_val, M)
        sse += ((pred - cvm.Y[val]) ** 2).sum(dim=1)
    return np.asarray(lambdas), torch.sqrt(sse / X.shape[0]).cpu().numpy(), nonzeros


def sklearn_cv_rmse(X, Y, labels, l1_ratio, lambdas):
    """The same numbers from scikit-learn refits on every training set (None without scikit-learn)."""
    try:
        from sklearn.linear_model import ElasticNet
    except ImportError:
        return None
    sse = np.zeros((len(lambdas), Y.shape[1]))
    for f in np.unique(labels):
        val, tr = labels == f, labels != f
        for l, lam in enumerate(lambdas):
            for m in range(Y.shape[1]):
                model = ElasticNet(alpha=lam / tr.sum(), l1_ratio=l1_ratio, fit_intercept=True, tol=1e-12,
                                   max_iter=100000).fit(X[tr], Y[tr, m])
                sse[l, m] += ((model.predict(X[val]) - Y[val, m]) ** 2).sum()
    return np.sqrt(sse / X.shape[0])


def main():
    N, K, M, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 2, 10)
    l1_ratio = float(sys.argv[5]) if len(sys.argv) >= 6 else 0.5
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, K)) + 0.3 * rng.standard_normal((N, 1))
    beta = np.zeros((K, M))
    for m in range(M):
        beta[rng.permutation(K)[:min(8, K)], m] = rng.uniform(0.5, 2.0, min(8, K)) * rng.choice([-1.0, 1.0], min(8, K))
    Y = X @ beta + 1.0 * rng.standard_normal((N, M))
    labels = np.arange(N) % P
    lambdas, rmse, nonzeros = fast_cv_rmse(X, Y, labels, l1_ratio)
    print(f"lambda        nonzeros   RMSE per response ({P}-fold cross-validation, l1_ratio = {l1_ratio:g})")
    for lam, row, nz in zip(lambdas, rmse, nonzeros):
        print(f"{lam:10.4g}  {nz.mean():8.1f}   " + "  ".join(f"{v:.5f}" for v in row))
    best = int(np.argmin(rmse.mean(axis=1)))
    print(f"lowest mean RMSE with lambda = {lambdas[best]:.4g} (alpha = lambda / n_train = "
          f"{lambdas[best] / (N - N // P):.4g} in scikit-learn's scale)")
    pick = sorted({1, len(lambdas) // 2, best})
    ref = sklearn_cv_rmse(X, Y, labels, l1_ratio, lambdas[pick])
    if ref is not None:
        worst = float(np.abs(rmse[pick] / ref - 1).max())
        print(f"against scikit-learn refits at lambda[{pick}]: largest relative RMSE difference {worst:.1e}")
        assert worst <= 1e-6, worst
    return rmse


if __name__ == "__main__":
    main()
