"""Helper of test_gpu_unions.py::test_uncompacted_partials_give_the_same_bits (run as a subprocess: the library
reads CVM_NO_COMPACT and CVM_FORCE_SPLITS once per process).  Writes the pair outputs of the split design,
formed from a sweep workspace that still holds every row split's partial, to the file named on the command
line, with the plan token's fields."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cvmatrix_amd as amd  # noqa: E402
import unions_cases as uc  # noqa: E402
from cvmatrix_amd.unions import fold_pairs  # noqa: E402


def main():
    X, Y, w, labels, _ = uc.split_design("float64")
    cvm = amd.CVMatrix(dtype=np.float64)
    cvm.fit(X, Y, w, folds=amd.Partitioner(labels))
    token = cvm._sweep[1]
    (xtx, xty), stats = cvm.training_XTX_XTY_unions(cvm.sweep_folds, fold_pairs(5))
    out = {n: t.cpu().numpy() for n, t in zip(("XTX", "XTY", "muX", "sdX", "muY", "sdY"), (xtx, xty) + tuple(stats))}
    np.savez(sys.argv[1], compacted=np.int64((token >> 40) & 1),
             plan=np.array([token & 0xfffff, (token >> 20) & 0xfffff], dtype=np.int64), **out)
    print("pairs written", xtx.shape)


if __name__ == "__main__":
    main()
