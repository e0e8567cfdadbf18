"""Fast cross-validation of principal component regression per number of components, end to end on one
MI355X.

    python examples/fast_cv_pcr.py [N K M folds]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY, means, stds of every fold          (HIP)
2. pcr_fit_batched                           eigenpairs of XtX and the coefficients on 1 .. A of them   (HIP)
3. pls_validation_sse                        squared validation errors of every fold's models          (HIP)
   -> RMSE per number of components, checked against scikit-learn refits (PCA + LinearRegression on every
   training set).  (Shapes whose device copies are padded -- odd K, float64 with odd M -- take the same
   formula in plain torch operations.)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.pcr import pcr_fit_batched  # noqa: E402
from cvmatrix_amd.pls import cv_rmse, pls_validation_sse  # noqa: E402


def fast_cv_rmse(X, Y, labels, A, weights=None):
    """RMSE[a, m] over all validation rows for PCR models with a+1 components on centred X and Y (an
    intercept), every row predicted by the model that was trained without its fold.  X, Y: NumPy arrays."""
    p = Partitioner(labels)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y, weights)
    batch = cvm.prepare_folds(p)
    (XTX, XTY), (muX, sdX, muY, sdY) = cvm.training_XTX_XTY_batched(batch)
    B = pcr_fit_batched(XTX, XTY, A, check=True).B                       # (F, A, K, M)
    if cvm._Kd == cvm._Ku and (cvm._Md or 0) == (cvm._Mu or 0):
        sse_f, wsum_f = pls_validation_sse(cvm, batch, (muX, sdX, muY, sdY), B)
        return cv_rmse(sse_f, wsum_f).cpu().numpy()
    sse = torch.zeros((B.shape[1], Y.shape[1]), dtype=torch.float64, device=B.device)
    wsum = 0.0
    for f, key in enumerate(p.folds_dict):
        val = torch.from_numpy(p.get_validation_indices(key)).to(B.device)
        pred = torch.matmul(cvm.X[val] - muX[f], B[f]) + muY[f]         # (A, n_val, M)
        err2 = (pred - cvm.Y[val]) ** 2
        if weights is not None:
            wv = cvm.weights[val]
            err2 = err2 * wv
            wsum += float(wv.sum())
        else:
            wsum += float(val.numel())
        sse += err2.sum(dim=1)
    return torch.sqrt(sse / wsum).cpu().numpy()


def sklearn_cv_rmse(X, Y, labels, A):
    """The same curve from scikit-learn refits on every training set (None without scikit-learn)."""
    try:
        from sklearn.decomposition import PCA
        from sklearn.linear_model import LinearRegression
    except ImportError:
        return None
    sse = np.zeros((A, Y.shape[1]))
    for f in np.unique(labels):
        tr, val = labels != f, labels == f
        for a in range(A):
            pca = PCA(n_components=a + 1, svd_solver="full").fit(X[tr])
            reg = LinearRegression().fit(pca.transform(X[tr]), Y[tr])
            sse[a] += ((reg.predict(pca.transform(X[val])) - Y[val]) ** 2).sum(axis=0)
    return np.sqrt(sse / X.shape[0])


def main():
    N, K, M, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 2, 10)
    rng = np.random.default_rng(0)
    L = rng.standard_normal((N, 6)) * np.array([6.0, 5.0, 4.0, 3.0, 2.0, 1.5])
    X = L @ np.linalg.qr(rng.standard_normal((K, 6)))[0].T + 0.2 * rng.standard_normal((N, K))
    Y = L[:, :3] @ rng.standard_normal((3, M)) + 0.1 * rng.standard_normal((N, M))
    A = min(K, 10)
    labels = np.arange(N) % P
    rmse = fast_cv_rmse(X, Y, labels, A)
    print(f"components  RMSE per response ({P}-fold cross-validation)")
    for a, row in enumerate(rmse):
        print(f"{a + 1:10d}  " + "  ".join(f"{v:.5f}" for v in row))
    best = int(np.argmin(rmse.mean(axis=1)))
    print(f"lowest mean RMSE with {best + 1} components")
    ref = sklearn_cv_rmse(X, Y, labels, A)
    if ref is None:
        print("scikit-learn is not installed: the curve was not checked against refits")
    else:
        err = float(np.max(np.abs(rmse - ref) / ref))
        print(f"scikit-learn refits (PCA + LinearRegression on every training set): largest relative difference {err:.1e}")
        assert err <= 1e-8, err
    return rmse


if __name__ == "__main__":
    main()
