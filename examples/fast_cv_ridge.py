"""Fast cross-validation of ridge regression over a grid of penalties, end to end on one MI355X.

    python examples/fast_cv_ridge.py [N K M folds]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY, means, stds of every fold   (HIP)
2. ridge_fit_batched                         (XtX + lambda I)^-1 XtY for every fold and lambda  (HIP)
3. pls_validation_sse                        squared validation errors of every fold's models    (HIP)
   -> RMSE per lambda.  (Shapes whose device copies are padded -- odd K, float64 with odd M -- take the
   same formula in plain torch operations.)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.pls import cv_rmse, pls_validation_sse  # noqa: E402
from cvmatrix_amd.ridge import ridge_fit_batched  # noqa: E402


def fast_cv_rmse(X, Y, labels, lambdas, weights=None):
    """RMSE[l, m] over all validation rows for ridge models with penalty lambdas[l] on centred X and Y
    (an intercept), every row predicted by the model that was trained without its fold.  X, Y: NumPy
    arrays."""
    p = Partitioner(labels)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y, weights)
    batch = cvm.prepare_folds(p)
    (XTX, XTY), (muX, sdX, muY, sdY) = cvm.training_XTX_XTY_batched(batch)
    B = ridge_fit_batched(XTX, XTY, lambdas).B                           # (F, L, K, M)
    if cvm._Kd == cvm._Ku and (cvm._Md or 0) == (cvm._Mu or 0):
        sse_f, wsum_f = pls_validation_sse(cvm, batch, (muX, sdX, muY, sdY), B)
        return cv_rmse(sse_f, wsum_f).cpu().numpy()
    sse = torch.zeros((B.shape[1], Y.shape[1]), dtype=torch.float64, device=B.device)
    wsum = 0.0
    for f, key in enumerate(p.folds_dict):
        val = torch.from_numpy(p.get_validation_indices(key)).to(B.device)
        pred = torch.matmul(cvm.X[val] - muX[f], B[f]) + muY[f]         # (L, n_val, M)
        err2 = (pred - cvm.Y[val]) ** 2
        if weights is not None:
            wv = cvm.weights[val]
            err2 = err2 * wv
            wsum += float(wv.sum())
        else:
            wsum += float(val.numel())
        sse += err2.sum(dim=1)
    return torch.sqrt(sse / wsum).cpu().numpy()


def main():
    N, K, M, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 2, 10)
    rng = np.random.default_rng(0)
    L = rng.standard_normal((N, 6))
    X = L @ rng.standard_normal((6, K)) + 0.2 * rng.standard_normal((N, K))
    Y = L[:, :3] @ rng.standard_normal((3, M)) + 0.1 * rng.standard_normal((N, M))
    lambdas = np.logspace(-3, 5, 17)
    rmse = fast_cv_rmse(X, Y, np.arange(N) % P, lambdas)
    print(f"lambda        RMSE per response ({P}-fold cross-validation)")
    for lam, row in zip(lambdas, rmse):
        print(f"{lam:10.3g}  " + "  ".join(f"{v:.5f}" for v in row))
    best = int(np.argmin(rmse.mean(axis=1)))
    print(f"lowest mean RMSE with lambda = {lambdas[best]:.3g}")
    return rmse


if __name__ == "__main__":
    main()
