"""The reference, the designs and the gates that tests/test_pcr_host.py (CPU) and tests/test_gpu_pcr.py (GPU)
hold the device PCR (cvm_pcr_fit) against.  Plain NumPy.

Gates (u = 2^-53, all normwise).  The kernel is a cyclic Jacobi iteration of at most 60 sweeps of K - 1
rounds; a round applies rotations that are orthogonal to a few u, so the computed decomposition is that
of a matrix within 60 K u ||G||_F of G:
  residual        ||G V_A - V_A L_A||_F   <= 60 K u ||G||_F
  orthogonality   ||V_A^T V_A - I||_F     <= 60 K u sqrt(A)
  eigenvalues     max |l_a - l_ref,a|     <= 60 K u ||G||_F          (Weyl)
Coefficients against the reference, ||B[a] - B_ref[a]||_F <= 1e-10 ||B_ref[a]||_F (the project's parity
bar), only where the split after component a+1 is well separated; float32 adds 2^-24 for the rounding of
the store.  Consistency, whatever the gaps: B[a] against the same sum rebuilt in float64 from the
kernel's own components and eigenvalues (the scores v_j^T H rounded once, see rebuild_coefficients),
<= 8 A u (l_1 / l_{a+1}) ||B[a]||_F."""

from fractions import Fraction

import numpy as np

U = 2.0 ** -53
PARITY = 1e-10
F32_STORE = 2.0 ** -24
MAX_SWEEPS = 60

GRID_K = (1, 2, 3, 7, 31, 32, 33, 64, 65, 96, 97, 129, 257)
GRID_M = (1, 3)
GRADED_K = (7, 33, 64, 129, 257)
CLUSTER_K = (7, 33, 129)


def default_rank_tol(K):
    return 32.0 * K * 2.0 ** -52


def backward_bound(K):
    return 60.0 * K * U


# ---------------------------------------------------------------------------------------------------------
# reference

def pcr_reference(G, H, A, rank_tol=None):
    """(B (A,K,M) or None, eigenvalues (A,), components (K,A), n_fit) of one fold from numpy.linalg.eigh in
    float64, eigenvalues descending, the rank rule and the cumulative formula of include/cvmhip.h."""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    tol = default_rank_tol(K) if rank_tol is None or rank_tol <= 0 else rank_tol
    lam, V = np.linalg.eigh(G)
    return reference_from_eig(lam[::-1], V[:, ::-1], H, A, tol)


def reference_from_eig(lam, V, H, A, tol):
    """The same from a decomposition in descending order (any eigensolver)."""
    n_fit = min(A, int(np.count_nonzero(lam > tol * lam[0])))
    comps = np.array(V[:, :A])
    comps[:, n_fit:] = 0.0
    B = None
    if H is not None:
        H = np.asarray(H, dtype=np.float64)
        H = H.reshape(H.shape[0], -1)
        B = np.zeros((A,) + H.shape)
        acc = np.zeros(H.shape)
        for a in range(A):
            if a < n_fit:
                acc = acc + np.outer(V[:, a], (V[:, a] @ H) / lam[a])
            B[a] = acc
    return B, np.array(lam[:A]), comps, n_fit


def exact_dot(v, H):
    """v^T H rounded once: the products and their sum in rational arithmetic."""
    v = [Fraction(float(x)) for x in v]
    return np.array([float(sum((x * Fraction(float(y)) for x, y in zip(v, H[:, m])), Fraction(0)))
                     for m in range(H.shape[1])])


def rebuild_coefficients(components, eigenvalues, H, n_fit):
    """sum_{j <= min(a, n_fit - 1)} v_j (v_j^T H) / l_j in float64 from a fit's own components and eigenvalues.
    The scores v_j^T H are rounded once (exact_dot): a component is a random direction to H, so their K products
    cancel, and a float64 dot product here carries K roundings of the largest partial sum into the rebuilt
    coefficients -- 79 u of ||B[0]|| at K = 257, M = 1 against the 64 u of the consistency gate, with the kernel's
    own sum compensated.  Everything after the scores is plain float64."""
    V = np.asarray(components, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    A = V.shape[1]
    B = np.zeros((A,) + H.shape)
    acc = np.zeros(H.shape)
    for a in range(A):
        if a < n_fit:
            acc = acc + np.outer(V[:, a], exact_dot(V[:, a], H) / eigenvalues[a])
        B[a] = acc
    return B


# ---------------------------------------------------------------------------------------------------------
# designs (each returns an exactly symmetric float64 matrix)

def sym(G):
    return 0.5 * (G + G.T)


def wishart(rng, K):
    X = rng.standard_normal((2 * K + 3, K))
    return sym(X.T @ X)


def low_rank(rng, K, r):
    X = rng.standard_normal((r, K))
    return sym(X.T @ X)


def orthogonal(rng, K):
    Q, R = np.linalg.qr(rng.standard_normal((K, K)))
    return Q * np.sign(np.diag(R))


def with_spectrum(rng, spectrum):
    Q = orthogonal(rng, len(spectrum))
    return sym((Q * np.asarray(spectrum, dtype=np.float64)) @ Q.T)


def graded(rng, K, ratio, rank=None):
    spec = float(ratio) ** -np.arange(K, dtype=np.float64)
    if rank is not None:
        spec[rank:] = 0.0
    return with_spectrum(rng, spec)


def clustered(rng, K):
    """Spectrum (9, 4, 4, 4, 1, ..., 1)."""
    spec = np.ones(K)
    spec[:4] = (9.0, 4.0, 4.0, 4.0)
    return with_spectrum(rng, spec)


def responses(rng, K, M):
    return rng.standard_normal((K, M))


# ---------------------------------------------------------------------------------------------------------
# gates

def align_signs(V, Vref):
    """V with every column's sign that of its dot product with the reference's column."""
    s = np.sign(np.sum(V * Vref, axis=0))
    s[s == 0] = 1.0
    return V * s


def sign_convention_holds(V, n_fit):
    """In every existing component the entry of largest magnitude is positive, the lowest index among equals."""
    for a in range(n_fit):
        k = int(np.argmax(np.abs(V[:, a])))          # (argmax: the first of equals)
        if not V[k, a] > 0:
            return False
    return True


def backward_figures(G, V, lam, lam_ref):
    """(residual / ||G||_F, orthogonality / sqrt(A), eigenvalue error / ||G||_F), each to be held to 60 K u."""
    G = np.asarray(G, dtype=np.float64)
    A = V.shape[1]
    nG = max(np.linalg.norm(G), np.finfo(np.float64).tiny)
    res = np.linalg.norm(G @ V - V * lam) / nG
    orth = np.linalg.norm(V.T @ V - np.eye(A)) / np.sqrt(A)
    eig = float(np.max(np.abs(lam - lam_ref))) / nG
    return res, orth, eig


def assert_backward(G, V, lam, lam_ref, what=""):
    K = G.shape[0]
    figs = backward_figures(G, V, lam, lam_ref)
    bound = backward_bound(K)
    for name, v in zip(("residual", "orthogonality", "eigenvalues"), figs):
        assert v <= bound, f"{what}: {name} {v:.3e} > 60 K u = {bound:.3e}"
    return figs


def coefficient_error(B, Bref):
    return float(np.linalg.norm(B - Bref) / max(np.linalg.norm(Bref), np.finfo(np.float64).tiny))


def assert_coefficients(B, Bref, comps, what="", float32=False):
    """Parity of B[a] for the components a in `comps`."""
    tol = PARITY + (F32_STORE if float32 else 0.0)
    worst = 0.0
    for a in comps:
        e = coefficient_error(np.asarray(B[a], dtype=np.float64), Bref[a])
        assert e <= tol, f"{what}: B[{a}] off by {e:.3e} > {tol:.3e}"
        worst = max(worst, e)
    return worst


def assert_consistency(B, V, lam, H, n_fit, what=""):
    """B[a] against the sum rebuilt from the fit's own V and eigenvalues; returns the largest err / bound."""
    A = V.shape[1]
    R = rebuild_coefficients(V, lam, H, n_fit)
    worst = 0.0
    for a in range(A):
        j = min(a, n_fit - 1)
        if j < 0:
            assert not np.any(B[a]), what
            continue
        bound = 8.0 * A * U * (lam[0] / lam[j]) * np.linalg.norm(B[a])
        e = np.linalg.norm(B[a] - R[a])
        assert e <= bound, f"{what}: B[{a}] inconsistent, {e:.3e} > {bound:.3e}"
        worst = max(worst, e / max(bound, np.finfo(np.float64).tiny))
    return worst
