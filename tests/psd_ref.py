"""A numpy restatement of the Higham projection the library computes in psd_mode 1 (sage_nearest_psd on the host,
sage_factor_psd_batch on the device), and the input families both are tested on.  No bump loop: the result may carry an
eigenvalue a few ulps below zero."""
import numpy as np

EPS = 2.0 ** -52
DIMS = (1, 2, 3, 29, 45, 46, 78, 80)
FAMILIES = ("gauge", "indefinite", "zeros", "rank_one", "scaled")
SEEDS = 6


def nearest_psd(M):
    """B = (M + M^T) / 2, H = V |w| V^T from numpy.linalg.eigh, (B + H) / 2 symmetrised"""
    M = np.asarray(M, np.float64)
    B = 0.5 * (M + M.T)
    w, V = np.linalg.eigh(B)
    H = (V * np.abs(w)) @ V.T
    A2 = 0.5 * (B + H)
    return 0.5 * (A2 + A2.T)


def symmetrised(M):
    M = np.asarray(M, np.float64)
    return 0.5 * (M + M.T)


def family(name, D, seed):
    """One fp32 [D, D] input:
    gauge       J^T J, J 400 x D with its first 7 columns a linear combination of the next 7 (D >= 14)
    indefinite  S + S^T, S Gaussian
    zeros       the no-inlier fallback
    rank_one    v v^T
    scaled      J^T J with column scales spread over 10^+-6"""
    r = np.random.default_rng([FAMILIES.index(name), D, seed])
    if name == "gauge":
        J = r.standard_normal((400, D)).astype(np.float32)
        if D >= 14:
            J[:, :7] = J[:, 7:14] @ r.standard_normal((7, 7)).astype(np.float32)
        return (J.T @ J).astype(np.float32)
    if name == "indefinite":
        S = r.standard_normal((D, D)).astype(np.float32)
        return (S + S.T).astype(np.float32)
    if name == "zeros":
        return np.zeros((D, D), np.float32)
    if name == "rank_one":
        v = r.standard_normal(D).astype(np.float32)
        return np.outer(v, v).astype(np.float32)
    if name == "scaled":
        J = r.standard_normal((400, D)) * 10.0 ** r.uniform(-6.0, 6.0, D)
        return (J.T @ J).astype(np.float32)
    raise ValueError(name)


def cases(D):
    """[(family, seed, M)] of one D: every family, SEEDS seeds each"""
    return [(name, seed, family(name, D, seed)) for name in FAMILIES for seed in range(SEEDS)]
