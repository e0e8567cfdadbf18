"""Nested (double) cross-validation of ridge regression on one MI355X: the penalty is selected per outer fold by
an inner cross-validation that never sees the outer fold, and the outer error is that of the selected models.

    python examples/nested_cv_ridge.py [N K M folds]

1. CVMatrix.fit(folds=...)                one sweep: full-data matrices + every fold's partials          (HIP)
2. training_XTX_XTY_unions(fold_pairs)    training matrices without folds f AND g, for every pair,
                                          from the partials -- no row of X is read again                 (HIP)
3. ridge_fit_batched + pls_validation_sse the pair models scored on the inner folds:
                                          unit (outer f, inner g) = model of pair {f, g} on the rows of g (HIP)
   -> inner RMSE per outer fold and penalty -> the penalty selected for each outer fold
4. training_XTX_XTY_batched + ridge + sse the single-fold models scored on their own fold, at the selected
                                          penalty -> the outer error
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402
from cvmatrix_amd.pls import pls_validation_sse  # noqa: E402
from cvmatrix_amd.ridge import ridge_fit_batched  # noqa: E402
from cvmatrix_amd.unions import fold_pairs, nested_units  # noqa: E402


def nested_cv_ridge(X, Y, labels, lambdas, weights=None):
    """Nested cross-validation of ridge models on centred X and Y (an intercept) over the folds of ``labels``.
    X, Y: NumPy arrays.  Returns a dict: ``inner_rmse`` (P, L) -- for outer fold f, the RMSE over the rows of
    all inner folds g != f (pooled over the responses) of the models trained without f and g; ``selected``
    (P,) the index of the penalty with the lowest inner RMSE; ``outer_sse`` (P, M) the squared errors of the
    model trained without f, at its selected penalty, on the rows of f; ``outer_wsum`` (P,) the weight of those
    rows; ``outer_rmse`` the error estimate of the whole procedure."""
    lambdas = np.asarray(lambdas, dtype=np.float64)
    p = Partitioner(labels)
    keys = list(p.folds_dict)
    P = len(keys)
    # (copy=False: the device copies keep the caller's K and M, which the scorer needs)
    cvm = CVMatrix(center_X=True, center_Y=True, scale_X=False, scale_Y=False, dtype=np.float64, copy=False)
    cvm.fit(X, Y, weights, folds=p)
    batch = cvm.sweep_folds
    dev = cvm.device
    # inner loop: one model per pair of folds and penalty, scored on both folds of the pair
    pairs = fold_pairs(P)
    (XTX2, XTY2), stats2 = cvm.training_XTX_XTY_unions(batch, pairs)
    B2 = ridge_fit_batched(XTX2, XTY2, lambdas).B                        # (pairs, L, K, M)
    outer, pair, inner = nested_units(P)
    arrays = [p.get_validation_indices(k) for k in keys]
    pidx = torch.from_numpy(pair).to(dev)
    unit_stats = tuple(None if s is None else s[pidx].contiguous() for s in stats2)
    sse_u, wsum_u = pls_validation_sse(cvm, [arrays[g] for g in inner], unit_stats, B2[pidx].contiguous())
    L, M = lambdas.size, sse_u.shape[2]
    oidx = torch.from_numpy(outer).to(dev)
    inner_sse = torch.zeros((P, L), dtype=torch.float64, device=dev).index_add_(0, oidx, sse_u.sum(dim=2))
    inner_w = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, oidx, wsum_u)
    inner_rmse = torch.sqrt(inner_sse / (inner_w[:, None] * M))
    selected = torch.argmin(inner_rmse, dim=1)
    # outer loop: the single-fold models at the selected penalties
    (XTX1, XTY1), stats1 = cvm.training_XTX_XTY_batched(batch)
    B1 = ridge_fit_batched(XTX1, XTY1, lambdas).B                        # (P, L, K, M)
    sse1, wsum1 = pls_validation_sse(cvm, batch, stats1, B1)             # (P, L, M), (P,)
    outer_sse = sse1[torch.arange(P, device=dev), selected]              # (P, M)
    outer_rmse = torch.sqrt(outer_sse.sum() / (wsum1.sum() * M))
    return {"inner_rmse": inner_rmse.cpu().numpy(), "selected": selected.cpu().numpy(),
            "outer_sse": outer_sse.cpu().numpy(), "outer_wsum": wsum1.cpu().numpy(), "outer_rmse": float(outer_rmse)}


def main():
    N, K, M, P = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (20000, 128, 2, 10)
    rng = np.random.default_rng(0)
    F = rng.standard_normal((N, 6))
    X = F @ rng.standard_normal((6, K)) + 0.2 * rng.standard_normal((N, K))
    Y = F[:, :3] @ rng.standard_normal((3, M)) + 0.1 * rng.standard_normal((N, M))
    lambdas = np.logspace(-3, 5, 17)
    res = nested_cv_ridge(X, Y, np.arange(N) % P, lambdas)
    print(f"outer fold   selected lambda   inner RMSE   ({P} x {P - 1} nested cross-validation)")
    for f in range(P):
        s = int(res["selected"][f])
        print(f"{f:10d}   {lambdas[s]:15.3g}   {res['inner_rmse'][f, s]:.5f}")
    print(f"outer RMSE of the selected models: {res['outer_rmse']:.5f}")
    return res


if __name__ == "__main__":
    main()
