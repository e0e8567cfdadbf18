"""Fast cross-validation of linear discriminant analysis over a grid of shrinkage values, end to end on one MI355X:
"how much shrinkage classifies best?"

    python examples/fast_cv_lda.py [N K C folds]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY (the class sums), means of every fold   (HIP)
2. lda_fit_batched                           within-class scatter by a rank-C downdate, one Cholesky solve
                                             per fold and shrinkage                                        (HIP)
3. lda_cv_predict                            every row's discriminants under the models trained without its
                                             fold (cv_predict), argmax                                     (HIP)
   -> cross-validated accuracy per shrinkage.  No row of X is read to fit a model.

Where scikit-learn is importable the accuracy is checked against LinearDiscriminantAnalysis(solver="lsqr",
shrinkage=g) refitted on every training set."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.lda import cv_lda, lda_cv_predict, raise_on_failure  # noqa: E402


def fast_cv_accuracy(X, y, labels, C, shrinkage):
    """(accuracy[l], predicted[N, l]): every row classified by the models that were trained without its fold.
    X: NumPy (N, K); y: class numbers 0 .. C-1; labels: the fold of every row."""
    Y = np.zeros((X.shape[0], C))
    Y[np.arange(X.shape[0]), y] = 1.0                                   # the class indicator, not scaled
    cvm = CVMatrix(center_X=True, center_Y=False, scale_X=False, scale_Y=False, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(Partitioner(labels))
    fit, stats = cv_lda(cvm, batch, shrinkage)
    raise_on_failure(fit, shrinkage)                                    # (the one wait for the device before the result)
    pred = lda_cv_predict(cvm, batch, stats, fit)                       # (N, L) int64
    truth = torch.from_numpy(y).to(pred.device)
    return (pred == truth[:, None]).to(torch.float64).mean(dim=0).cpu().numpy(), pred.cpu().numpy()


def sklearn_cv_predictions(X, y, labels, shrinkage):
    """The same predictions from scikit-learn refits on every training set (None without scikit-learn)."""
    try:
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    except ImportError:
        return None
    pred = np.empty((X.shape[0], len(shrinkage)), dtype=np.int64)
    for f in np.unique(labels):
        val, tr = labels == f, labels != f
        for l, g in enumerate(shrinkage):
            pred[val, l] = LinearDiscriminantAnalysis(solver="lsqr", shrinkage=float(g)).fit(X[tr], y[tr]).predict(X[val])
    return pred


def main():
    N, K, C, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 5, 10)
    rng = np.random.default_rng(0)
    y = rng.integers(0, C, N)
    means = rng.standard_normal((C, K)) * (2.5 / np.sqrt(K))
    mix = np.eye(K) + 0.5 * rng.standard_normal((K, K)) / np.sqrt(K)    # correlated variables
    X = (rng.standard_normal((N, K)) + means[y]) @ mix + 0.3
    labels = np.arange(N) % P
    shrinkage = np.array([0.0, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 1.0])
    acc, pred = fast_cv_accuracy(X, y, labels, C, shrinkage)
    print(f"shrinkage   accuracy ({P}-fold cross-validation, {C} classes)")
    for g, a in zip(shrinkage, acc):
        print(f"{g:9.2f}   {a:.5f}")
    print(f"best accuracy with shrinkage {shrinkage[int(np.argmax(acc))]:g}")
    ref = sklearn_cv_predictions(X, y, labels, shrinkage)
    if ref is not None:
        differ = (pred != ref).mean(axis=0)
        ref_acc = (ref == y[:, None]).mean(axis=0)
        print("against scikit-learn refits: share of rows labelled differently per shrinkage "
              + " ".join(f"{d:.1e}" for d in differ) + f"; largest accuracy difference {np.abs(acc - ref_acc).max():.1e}")
        # a row changes its label only where its two best discriminants agree to rounding: a handful in a million
        assert differ.max() <= 1e-4 and np.abs(acc - ref_acc).max() <= 1e-4, (differ, acc, ref_acc)
    return acc


if __name__ == "__main__":
    main()
