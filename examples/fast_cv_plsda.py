"""Fast cross-validation of a PLS-DA classifier, end to end on one MI355X: PLS regression on one-hot class
indicators, every row classified by the models that were trained without its fold.

    python examples/fast_cv_plsda.py [N K classes folds components]

1. CVMatrix.fit + training_XTX_XTY_batched   training-set XtX, XtY, means, stds of every fold        (HIP)
2. pls_fit_batched                           A-component PLS coefficients of every fold               (HIP)
3. cv_predict                                the out-of-fold scores of every row, (N, A, classes)     (HIP)
   -> class = argmax over the responses; cross-validated accuracy per number of components.
The decisions are checked against scikit-learn refits (PLSRegression on every training set, for every number
of components) where scikit-learn is installed, against a float64 torch loop over the folds otherwise: the
same class for every row whose two highest reference scores lie further apart than the scores can differ.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.pls import pls_fit_batched  # noqa: E402
from cvmatrix_amd.predict import cv_predict  # noqa: E402


def fast_cv_scores(X, Y, labels, A):
    """Out-of-fold scores (N, A, classes) on the device, and what the check below needs."""
    p = Partitioner(labels)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=True, scale_Y=True, ddof=1, dtype=np.float64)
    cvm.fit(X, Y)
    batch = cvm.prepare_folds(p)
    (XTX, XTY), stats = cvm.training_XTX_XTY_batched(batch)
    B = pls_fit_batched(XTX, XTY, A).B                                   # (F, A, K, classes)
    return cv_predict(cvm, batch, stats, B), (cvm, p, stats, B)


def torch_loop_scores(cvm, p, stats, B):
    """The same scores by one gather and one matmul per fold, and the bound on what the device's rounding
    can move a score by: 2 (K + 8) u |z| . |b| |sdY| + 2 u |score|, u = 2^-53 (tests/predict_cases.py)."""
    muX, sdX, muY, sdY = stats
    F, A, K, M = B.shape
    ref = torch.empty((cvm.N, A, M), dtype=torch.float64, device=B.device)
    gate = torch.empty_like(ref)
    u = 2.0 ** -53
    for f, key in enumerate(p.folds_dict):
        val = torch.from_numpy(p.get_validation_indices(key)).to(B.device)
        z = (cvm.X[val] - muX[f]) / sdX[f]
        s = (torch.matmul(z, B[f]) * sdY[f] + muY[f]).transpose(0, 1)
        S = torch.matmul(z.abs(), B[f].abs()).transpose(0, 1)
        ref[val] = s
        gate[val] = 2 * (K + 8) * u * S * sdY[f].abs() + 2 * u * s.abs()
    return ref, gate


def sklearn_scores(X, Y, labels, A):
    """Refits: PLSRegression on every training set for every number of components (None without scikit-learn)."""
    try:
        from sklearn.cross_decomposition import PLSRegression
    except ImportError:
        return None
    ref = np.empty((X.shape[0], A, Y.shape[1]))
    for f in np.unique(labels):
        tr, val = labels != f, labels == f
        for a in range(A):
            ref[val, a] = PLSRegression(n_components=a + 1, scale=True, tol=1e-12, max_iter=5000).fit(X[tr], Y[tr]).predict(X[val])
    return ref


def same_decisions(scores, ref, margin):
    """Every row whose two highest reference scores differ by more than `margin` gets the reference's class.
    Returns (rows compared, rows too close to call)."""
    top = np.sort(ref, axis=-1)
    clear = top[..., -1] - top[..., -2] > margin
    agree = scores.argmax(-1) == ref.argmax(-1)
    assert agree[clear].all(), f"{int((~agree & clear).sum())} clear decisions differ"
    return int(clear.sum()), int((~clear).sum())


def main():
    N, K, C, P, A = (int(a) for a in sys.argv[1:6]) if len(sys.argv) >= 6 else (3000, 40, 3, 5, 6)
    rng = np.random.default_rng(0)
    cls = rng.integers(0, C, N)
    centres = rng.standard_normal((C, 4)) * 1.5
    L = centres[cls] + rng.standard_normal((N, 4))
    X = L @ rng.standard_normal((4, K)) + 0.5 * rng.standard_normal((N, K))
    Y = np.eye(C)[cls]                                                   # one-hot responses
    labels = np.arange(N) % P
    scores_d, (cvm, p, stats, B) = fast_cv_scores(X, Y, labels, A)
    scores = scores_d.cpu().numpy()
    acc = (scores.argmax(-1) == cls[:, None]).mean(axis=0)
    print(f"components  accuracy ({P}-fold cross-validation, {C} classes)")
    for a in range(A):
        print(f"{a + 1:10d}  {acc[a]:.4f}")
    print(f"highest accuracy with {int(acc.argmax()) + 1} components")
    # the device's rounding: twice the bound per score (either of the two highest may move)
    ref_t, gate_t = torch_loop_scores(cvm, p, stats, B)
    margin = 2 * gate_t.max(dim=-1).values.cpu().numpy()
    n, close = same_decisions(scores, ref_t.cpu().numpy(), margin)
    print(f"float64 torch loop over the folds: {n} decisions the same, {close} too close to call")
    ref = sklearn_scores(X, Y, labels, A)
    if ref is None:
        print("scikit-learn is not installed: the decisions were not checked against refits")
    else:
        # (another algorithm for the weights -- NIPALS' power iteration against the kernel algorithm's repeated
        #  squaring: the two MODELS differ, most in the late components.  How far is measured between the two
        #  references, per number of components, with no prediction of the device in it, and either of the two
        #  highest scores may move by that much on top of the rounding)
        apart = np.abs(ref - ref_t.cpu().numpy()).max(axis=(0, 2))
        n, close = same_decisions(scores, ref, margin + 2 * apart)
        print(f"scikit-learn refits on every training set: {n} decisions the same, {close} too close to call; "
              f"the refits' scores and the float64 loop's at most {apart.max():.1e} apart")
    return acc


if __name__ == "__main__":
    main()
