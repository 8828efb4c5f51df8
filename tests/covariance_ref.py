"""fp64 restatement of the marginal covariances (include/sage_ba.h "marginal covariances"): numpy.linalg.inv of the dense
system, and the depth variance j'Sj per pixel.  No engine code."""
import numpy as np

EPS = 2.0 ** -53


def damped(H, damp):
    """(H) + damp diag(H): what sage_block_solve factorises once the diagonal priors are in H"""
    return H + damp * np.diag(np.diag(H))


def dense_from_blocks(K, B, diag, links, link_blocks, diag_add=None):
    """the symmetric [K B, K B] matrix of diagonal blocks [K,B,B] and link blocks [n,B,B] (rows links[.][0]); a link listed
    twice is summed"""
    H = np.zeros((K * B, K * B))
    for k in range(K):
        H[k * B:(k + 1) * B, k * B:(k + 1) * B] = diag[k]
    for (a, b), L in zip(links, link_blocks):
        H[a * B:(a + 1) * B, b * B:(b + 1) * B] += L
        H[b * B:(b + 1) * B, a * B:(a + 1) * B] += L.T
    if diag_add is not None:
        H = H + np.diag(np.asarray(diag_add, np.float64).reshape(-1))
    return H


def covariance(M):
    """Sigma = M^-1, cond_2(M), ||Sigma||_2"""
    M = np.asarray(M, np.float64)
    Sigma = np.linalg.inv(M)
    sv = np.linalg.svd(M, compute_uv=False)
    return Sigma, float(sv[0] / sv[-1]), float(1.0 / sv[-1])


def bar(n, cond, norm2):
    """||Sigma_hat - Sigma||_F <= 64 n 2^-53 cond_2(M) ||Sigma||_2 for every block: the backward error of an n-row Cholesky
    factor carried through the inverse, the form tests/test_gpu_marginal_prior.py uses for the Schur complement"""
    return 64.0 * n * EPS * cond * norm2


def block(Sigma, B, a, b):
    return Sigma[a * B:(a + 1) * B, b * B:(b + 1) * B]


def gamma(N):
    u = 2.0 ** -24
    return N * u / (1.0 - N * u)


def depth_variance(bias, basis, code, scale, S):
    """var64 [HW] = j'Sj from the fp32-rounded inputs in fp64, and the magnitude |j|'|S||j| with |j| built from
    |bias| + |basis||code| that the rounding bound scales with"""
    bias = np.asarray(bias, np.float32).astype(np.float64); basis = np.asarray(basis, np.float32).astype(np.float64)
    code = np.asarray(code, np.float32).astype(np.float64); s = float(np.float32(scale))
    S = np.asarray(S, np.float64)
    S = (0.5 * (S + S.T)).astype(np.float32).astype(np.float64)
    j = np.concatenate([s * basis, (bias + basis @ code)[:, None]], axis=1)
    ja = np.concatenate([abs(s) * np.abs(basis), (np.abs(bias) + np.abs(basis) @ np.abs(code))[:, None]], axis=1)
    return np.einsum("pi,ij,pj->p", j, S, j), np.einsum("pi,ij,pj->p", ja, np.abs(S), ja)
