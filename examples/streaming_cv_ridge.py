"""Cross-validated ridge regression over data that is read in chunks: no more than one chunk of rows is on the
device at any time.

    python examples/streaming_cv_ridge.py [N K M folds chunks]

Pass 1  StreamingCVMatrix.partial_fit per chunk   every fold's X'X, X'Y, column sums accumulated        (HIP)
        training_XTX_XTY_batched                  training-set matrices, means of every fold            (HIP)
        ridge_fit_batched                         (X'X + lambda I)^-1 X'Y for every fold and lambda     (HIP)
Pass 2  per chunk: pls_validation_sse             squared errors of every fold's models on the fold's
                                                  rows OF THE CHUNK; sse and wsum are summed over chunks (HIP)
        -> RMSE per lambda.
Every chunk must hold rows of every fold (the scorer cuts every fold of a chunk into row pieces)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, StreamingCVMatrix  # noqa: E402
from cvmatrix_amd.pls import pls_validation_sse  # noqa: E402
from cvmatrix_amd.ridge import ridge_fit_batched  # noqa: E402


def streaming_cv_rmse(chunks, P, lambdas):
    """RMSE[l, m] over all validation rows for ridge models with penalty lambdas[l] on centred X and Y (an
    intercept), every row predicted by the model trained without its fold.  ``chunks()`` returns an iterator of
    ``(X, Y, weights | None, labels)`` NumPy chunks, labels in [0, P); it is called twice (two passes over the
    data)."""
    scv = StreamingCVMatrix(P, center_X=True, center_Y=True, dtype=np.float64)
    for Xc, Yc, wc, lab in chunks():
        scv.partial_fit(Xc, Yc, wc, lab)
    (XTX, XTY), stats = scv.training_XTX_XTY_batched()
    B = ridge_fit_batched(XTX, XTY, lambdas).B                           # (P, L, K, M)
    sse, wsum = None, None
    for Xc, Yc, wc, lab in chunks():
        lab = np.asarray(lab)
        cvm_c = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64, copy=False,
                         lazy_fit=True)                                  # (holds the chunk; its own Gram is never formed)
        cvm_c.fit(Xc, Yc, wc)
        s, ws_ = pls_validation_sse(cvm_c, [np.flatnonzero(lab == f) for f in range(P)], stats, B)
        sse = s.sum(dim=0) if sse is None else sse + s.sum(dim=0)
        wsum = ws_.sum() if wsum is None else wsum + ws_.sum()
    return torch.sqrt(sse / wsum).cpu().numpy()


def main():
    N, K, M, P, C = (int(a) for a in sys.argv[1:6]) if len(sys.argv) >= 6 else (20000, 128, 2, 10, 4)
    rng = np.random.default_rng(0)
    L = rng.standard_normal((N, 6))
    X = L @ rng.standard_normal((6, K)) + 0.2 * rng.standard_normal((N, K))
    Y = L[:, :3] @ rng.standard_normal((3, M)) + 0.1 * rng.standard_normal((N, M))
    labels = np.arange(N) % P
    bounds = np.linspace(0, N, C + 1).astype(int)

    def chunks():                                       # (stands for a reader of files)
        for a, b in zip(bounds[:-1], bounds[1:]):
            yield X[a:b], Y[a:b], None, labels[a:b]
    lambdas = np.logspace(-3, 5, 17)
    rmse = streaming_cv_rmse(chunks, P, lambdas)
    print(f"lambda        RMSE per response ({P}-fold cross-validation, {C} chunks)")
    for lam, row in zip(lambdas, rmse):
        print(f"{lam:10.3g}  " + "  ".join(f"{v:.5f}" for v in row))
    best = int(np.argmin(rmse.mean(axis=1)))
    print(f"lowest mean RMSE with lambda = {lambdas[best]:.3g}")
    return rmse


if __name__ == "__main__":
    main()
