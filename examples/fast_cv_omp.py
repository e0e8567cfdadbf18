"""Fast cross-validation of forward variable selection (orthogonal matching pursuit) over the number of selected
variables, end to end on one MI355X: "which 5, 10 or 20 variables, and how many?"

    python examples/fast_cv_omp.py [N K M folds [A]]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY, means, stds of every fold        (HIP)
2. omp_fit_batched                           greedy selection on (XtX, XtY) for every fold and response,
                                             least-squares refit after every selection                 (HIP)
3. pls_validation_sse                        squared validation errors of every fold's models          (HIP)
   -> RMSE per number of selected variables.  (Shapes whose device copies are padded -- odd K, float64 with
   odd M -- take the same formula in plain torch operations.)

Where scikit-learn is importable the RMSE is checked against OrthogonalMatchingPursuit(n_nonzero_coefs=a,
fit_intercept=True) refitted on every training set (= centring with the training means)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.omp import omp_fit_batched  # noqa: E402
from cvmatrix_amd.pls import cv_rmse, pls_validation_sse  # noqa: E402


def fast_cv_rmse(X, Y, labels, A, normalize=False):
    """(RMSE[a, m], support[f, a, m]): RMSE over all validation rows for the least-squares models on the first
    a+1 selected variables of centred X and Y (an intercept), every row predicted by the model that was trained
    without its fold; support: the variable each fold's path selected at step a (-1: the path had ended).
    X, Y: NumPy arrays."""
    p = Partitioner(labels)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(p)
    (XTX, XTY), (muX, sdX, muY, sdY) = cvm.training_XTX_XTY_batched(batch)
    fit = omp_fit_batched(XTX, XTY, A, normalize=normalize, check=True)           # B (F, A, K, M)
    support = fit.support.cpu().numpy()
    if cvm._Kd == cvm._Ku and (cvm._Md or 0) == (cvm._Mu or 0):
        sse_f, wsum_f = pls_validation_sse(cvm, batch, (muX, sdX, muY, sdY), fit.B)
        return cv_rmse(sse_f, wsum_f).cpu().numpy(), support
    sse = torch.zeros((A, Y.shape[1]), dtype=torch.float64, device=fit.B.device)
    for f, key in enumerate(p.folds_dict):
        val = torch.from_numpy(p.get_validation_indices(key)).to(fit.B.device)
        pred = torch.matmul(cvm.X[val] - muX[f], fit.B[f]) + muY[f]         # (A, n_val, M)
        sse += ((pred - cvm.Y[val]) ** 2).sum(dim=1)
    return torch.sqrt(sse / X.shape[0]).cpu().numpy(), support


def sklearn_cv_rmse(X, Y, labels, A):
    """The same numbers from scikit-learn refits on every training set (None without scikit-learn)."""
    try:
        from sklearn.linear_model import OrthogonalMatchingPursuit
    except ImportError:
        return None
    sse = np.zeros((A, Y.shape[1]))
    for f in np.unique(labels):
        val, tr = labels == f, labels != f
        for a in range(A):
            for m in range(Y.shape[1]):
                model = OrthogonalMatchingPursuit(n_nonzero_coefs=a + 1, fit_intercept=True).fit(X[tr], Y[tr, m])
                sse[a, m] += ((model.predict(X[val]) - Y[val, m]) ** 2).sum()
    return np.sqrt(sse / X.shape[0])


def main():
    N, K, M, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 2, 10)
    A = int(sys.argv[5]) if len(sys.argv) >= 6 else min(K, 16)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, K)) + 0.3 * rng.standard_normal((N, 1))
    beta = np.zeros((K, M))
    for m in range(M):
        beta[rng.permutation(K)[:min(8, K)], m] = rng.uniform(0.5, 2.0, min(8, K)) * rng.choice([-1.0, 1.0], min(8, K))
    Y = X @ beta + 1.0 * rng.standard_normal((N, M))
    labels = np.arange(N) % P
    rmse, support = fast_cv_rmse(X, Y, labels, A)
    print(f"variables   RMSE per response ({P}-fold cross-validation)   selected at this step in fold 0")
    for a, row in enumerate(rmse):
        print(f"{a + 1:9d}   " + "  ".join(f"{v:.5f}" for v in row) + "   " + " ".join(str(v) for v in support[0, a]))
    best = int(np.argmin(rmse.mean(axis=1)))
    print(f"lowest mean RMSE with {best + 1} variables")
    ref = sklearn_cv_rmse(X, Y, labels, min(A, 4))
    if ref is not None:
        worst = float(np.abs(rmse[:ref.shape[0]] / ref - 1).max())
        print(f"against scikit-learn refits with 1 .. {ref.shape[0]} variables: largest relative RMSE difference {worst:.1e}")
        assert worst <= 1e-8, worst
    return rmse


if __name__ == "__main__":
    main()
