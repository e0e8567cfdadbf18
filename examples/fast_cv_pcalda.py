"""Fast cross-validation of PCA-LDA over the number of principal components, end to end on one MI355X:
"how many components classify best?"

    python examples/fast_cv_pcalda.py [N K C folds A]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY (the class sums), means of every fold   (HIP)
2. pcalda_fit_batched                        the A leading eigenpairs of every fold, then one A x A Cholesky
                                             factorisation per fold gives the discriminants on 1 .. A
                                             components                                                    (HIP)
3. lda_cv_predict                            every row's discriminants under the models trained without its
                                             fold (cv_predict), argmax                                     (HIP)
   -> cross-validated accuracy per number of components.  No row of X is read to fit a model.

Where scikit-learn is importable the accuracy is checked against Pipeline(PCA(a), LinearDiscriminantAnalysis(
solver="lsqr")) refitted on every training set."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.lda import lda_cv_predict  # noqa: E402
from cvmatrix_amd.pcalda import cv_pcalda, raise_on_failure  # noqa: E402


def fast_cv_accuracy(X, y, labels, C, A, solver="scalar"):
    """(accuracy[a], predicted[N, a]): every row classified by the models that were trained without its fold.
    X: NumPy (N, K); y: class numbers 0 .. C-1; labels: the fold of every row."""
    Y = np.zeros((X.shape[0], C))
    Y[np.arange(X.shape[0]), y] = 1.0                                   # the class indicator, not scaled
    cvm = CVMatrix(center_X=True, center_Y=False, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(Partitioner(labels))
    fit, stats = cv_pcalda(cvm, batch, A, solver=solver)
    raise_on_failure(fit)                                               # (the one wait for the device before the result)
    pred = lda_cv_predict(cvm, batch, stats, fit)                       # (N, A) int64
    truth = torch.from_numpy(y).to(pred.device)
    return (pred == truth[:, None]).to(torch.float64).mean(dim=0).cpu().numpy(), pred.cpu().numpy()


def sklearn_cv_predictions(X, y, labels, A):
    """The same predictions from scikit-learn refits on every training set (None without scikit-learn)."""
    try:
        from sklearn.decomposition import PCA
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
        from sklearn.pipeline import make_pipeline
    except ImportError:
        return None
    pred = np.empty((X.shape[0], A), dtype=np.int64)
    for f in np.unique(labels):
        val, tr = labels == f, labels != f
        for a in range(A):
            pipe = make_pipeline(PCA(a + 1, svd_solver="full"), LinearDiscriminantAnalysis(solver="lsqr"))
            pred[val, a] = pipe.fit(X[tr], y[tr]).predict(X[val])
    return pred


def main():
    N, K, C, P, A = (int(a) for a in sys.argv[1:6]) if len(sys.argv) >= 6 else (20000, 128, 5, 10, 16)
    rng = np.random.default_rng(0)
    y = rng.integers(0, C, N)
    s = 0.9 ** np.arange(K)                                             # a decaying spectrum: the components are determined
    means = 1.5 * rng.standard_normal((C, K)) * s
    mix = np.linalg.qr(rng.standard_normal((K, K)))[0]                  # correlated variables
    X = (rng.standard_normal((N, K)) * s + means[y]) @ mix + 0.3
    labels = np.arange(N) % P
    acc, pred = fast_cv_accuracy(X, y, labels, C, A)
    print(f"components   accuracy ({P}-fold cross-validation, {C} classes)")
    for a, v in enumerate(acc):
        print(f"{a + 1:10d}   {v:.5f}")
    print(f"best accuracy with {int(np.argmax(acc)) + 1} components")
    ref = sklearn_cv_predictions(X, y, labels, A)
    if ref is not None:
        differ = (pred != ref).mean(axis=0)
        ref_acc = (ref == y[:, None]).mean(axis=0)
        print("against scikit-learn refits: share of rows labelled differently per number of components "
              + " ".join(f"{d:.1e}" for d in differ) + f"; largest accuracy difference {np.abs(acc - ref_acc).max():.1e}")
        # a row changes its label only where its two best discriminants agree to rounding: a handful in a million
        assert differ.max() <= 1e-4 and np.abs(acc - ref_acc).max() <= 1e-4, (differ, acc, ref_acc)
    return acc


if __name__ == "__main__":
    main()
