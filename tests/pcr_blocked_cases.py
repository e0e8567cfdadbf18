"""The NumPy model of the blocked device eigensolver (cvm_pcr_blocked_fit, csrc/pcr_blocked.hpp) and the shapes
tests/test_pcr_blocked_host.py (CPU) and tests/test_gpu_pcr_blocked.py (GPU) run it at, written in terms of the
block size b.  The gates, the designs and the reference are those of tests/pcr_cases.py, unchanged.

The model is the method, not the kernel's bits: cyclic two-sided block Jacobi, blocks of b indices, the
round-robin order of the scalar kernel applied to blocks, ONE cyclic scalar Jacobi sweep on the 2b x 2b
subproblem of every pair per visit, pair (p, q) rotating iff |S_pq| > 2^-52 ||G||_F.  The matrix is padded with
zeros to an even number of whole blocks; a padded index never rotates (its off-diagonal entries are exactly 0),
and the padding block is paired like any other so that its partner still sweeps its own diagonal block."""

import numpy as np

MAX_SWEEPS = 60


def round_robin_pair(r, i, m):
    """Pair i of round r among m players (m even): (m-1, r) and ((r+i) mod (m-1), (r-i) mod (m-1)), p < q."""
    u = m - 1 if i == 0 else (r + i) % (m - 1)
    v = r if i == 0 else (r - i) % (m - 1)
    return (u, v) if u < v else (v, u)


def blocks_even(K, b):
    """The number of blocks, rounded up to even."""
    nb = -(-K // b)
    return (nb + 1) & ~1


def inner_sweep(T, thr):
    """One cyclic Jacobi sweep (round-robin, n - 1 rounds of n / 2 disjoint rotations) on the symmetric T.
    Returns (Q, Q^T T Q, a rotation was made)."""
    n = T.shape[0]
    T = T.copy()
    Q = np.eye(n)
    rotated = False
    for r in range(n - 1):
        pq = np.array([round_robin_pair(r, i, n) for i in range(n // 2)])
        p, q = pq[:, 0], pq[:, 1]
        spq = T[p, q]
        rot = np.abs(spq) > thr
        if not rot.any():
            continue
        rotated = True
        p, q, spq = p[rot], q[rot], spq[rot]
        zeta = (T[q, q] - T[p, p]) / (2.0 * spq)
        t = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = c * t
        J = np.eye(n)
        J[p, p] = c
        J[q, q] = c
        J[p, q] = s
        J[q, p] = -s
        dp, dq = T[p, p] - t * spq, T[q, q] + t * spq
        T = J.T @ T @ J
        T = 0.5 * (T + T.T)
        T[p, q] = T[q, p] = 0.0
        T[p, p], T[q, q] = dp, dq
        Q = Q @ J
    return Q, T, rotated


def block_jacobi_model(G, b, max_sweeps=MAX_SWEEPS):
    """(eigenvalues descending (K,), V (K,K) in that order, sweeps) of the symmetric G by the method above;
    sweeps counts the last sweep, which makes no rotation; -1 if max_sweeps did not suffice."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    m = blocks_even(K, b)
    Kp = m * b
    S = np.zeros((Kp, Kp))
    S[:K, :K] = G
    V = np.eye(Kp)
    thr = 2.0 ** -52 * np.linalg.norm(G)
    off = ~np.eye(2 * b, dtype=bool)
    sweeps = -1
    for sweep in range(1, max_sweeps + 1):
        rotated = False
        for r in range(m - 1):
            for i in range(m // 2):
                I, J = round_robin_pair(r, i, m)
                idx = np.r_[I * b:(I + 1) * b, J * b:(J + 1) * b]
                T = S[np.ix_(idx, idx)]
                if not np.any(np.abs(T[off]) > thr):
                    continue
                Q, T, rot = inner_sweep(T, thr)
                if not rot:
                    continue
                rotated = True
                S[:, idx] = S[:, idx] @ Q
                S[idx, :] = Q.T @ S[idx, :]
                S[np.ix_(idx, idx)] = T
                V[:, idx] = V[:, idx] @ Q
        if not rotated:
            sweeps = sweep
            break
    lam = np.diag(S)[:K]
    order = np.argsort(-lam, kind="stable")
    return lam[order], V[:K, :K][:, order], sweeps


# ---------------------------------------------------------------------------------------------------------
# shapes, in terms of the block size

def grid_K(b):
    """One block, one exact pair, a ragged last block of one column, an odd number of blocks, padding."""
    return (1, 2, b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, 3 * b, 4 * b + 1, 5 * b + 3)


GRID_M = (1, 3)


def host_K(b):
    return (b + 1, 2 * b + 1, 129)


def graded_K(b):
    return (b + 1, 129, 257)


PAST_OLD_LIMIT = ((513, 2, 16, 2), (640, 2, 8, 2), (1024, 2, 16, 2))      # (K, F, A, M)
