"""fp64 numpy restatement of teaser::RobustRegistrationSolver::solve(src, dst, noise_bounds) in the reference's shipped
configuration (inlier_selection_mode none, chain TIMs, GNC-TLS, estimate_scaling), operation by operation
(thirdparty/TEASER-plusplus/teaser/src/registration.cc:21-88, :297-313, :361-388, :395-485, :586-690, :990-1101;
include/teaser/utils.h:121-136).  Test infrastructure: the engine's device vote and host finish are compared against it, and
it against fixtures the reference's own code wrote (tests/golden/registration_*.npz).

The running sums of the vote are sequential (``block=None``: np.cumsum adds left to right, as the reference's loop does) or
in another order (``block=k``: sums inside blocks of k endpoints, then over the blocks -- the shape of a device scan).  Every
function also returns the margins of the discrete decisions it takes, so a test can show that no rounding difference flips
one.  The one deliberate difference of the engine is restated too: pairs without a usable measurement (|src_j - src_i| = 0)
leave the vote (``degenerate``)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53


def pair_measurements(src, dst, nb, cbar2=1.0):
    """-> X, r [pairs] in the reference's pair order (i < j; i * N - i (i + 1) / 2 + j - i - 1), i, j, degenerate [pairs]"""
    src = np.asarray(src, np.float64); dst = np.asarray(dst, np.float64); nb = np.asarray(nb, np.float64)
    N = src.shape[0]
    i, j = np.triu_indices(N, 1)
    ds = src[j] - src[i]; dd = dst[j] - dst[i]
    sq = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    v1 = np.sqrt(sq(ds)); v2 = np.sqrt(sq(dd))
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v2 / v1
        r = ((nb[j] + nb[i]) * np.sqrt(cbar2)) * (1.0 / v1)
        w = 1.0 / (r * r)
    degenerate = ~((v1 > 0) & np.isfinite(X) & np.isfinite(r) & (r > 0) & np.isfinite(w))
    return X, r, i, j, degenerate


def _prefix(terms, block):
    if block is None:
        return np.cumsum(terms)
    n = terms.size
    pad = (-n) % block
    t = np.concatenate([terms, np.zeros(pad)]).reshape(-1, block)
    inner = np.cumsum(t, axis=1)
    offs = np.concatenate([[0.0], np.cumsum(inner[:, -1])[:-1]])
    return (offs[:, None] + inner).reshape(-1)[:n]


def tls_estimate(X, ranges, block=None):
    """ScalarTLSEstimator::estimate.  -> dict(estimate, inliers, cost (the minimum), min_index, costs, x_hats, keys (sorted),
    eps, idx (per sorted endpoint), second_gap (second-lowest cost - lowest), ties (equal neighbouring keys))"""
    X = np.asarray(X, np.float64); ranges = np.asarray(ranges, np.float64)
    n = X.size
    h = np.empty(2 * n); h[0::2] = X - ranges; h[1::2] = X + ranges
    sign = np.empty(2 * n); sign[0::2] = 1.0; sign[1::2] = -1.0
    owner = np.repeat(np.arange(n), 2)
    order = np.argsort(h, kind="stable")
    keys, eps, idx = h[order], sign[order], owner[order]
    w = 1.0 / (ranges * ranges)
    ew = eps * w[idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        s_w = _prefix(ew, block)
        s_wx = _prefix(ew * X[idx], block)
        s_r = _prefix(eps * ranges[idx], block)
        s_x = _prefix(eps * X[idx], block)
        s_xx = _prefix((eps * X[idx]) * X[idx], block)
        card = np.cumsum(eps)
        r_all = float(np.cumsum(ranges)[-1])
        x_hat = s_wx / s_w
        cost = (card * x_hat) * x_hat + s_xx - (2 * s_x) * x_hat + (r_all - s_r)
    finite = np.where(np.isnan(cost), np.inf, cost)
    k = int(np.argmin(finite))          # the first smallest; a NaN never wins
    est = float(x_hat[k])
    others = np.delete(finite, k)
    second_gap = float(others.min() - finite[k]) if others.size else np.inf
    return dict(estimate=est, inliers=np.abs(X - est) <= ranges, cost=float(cost[k]), min_index=k, costs=cost, x_hats=x_hat,
                keys=keys, eps=eps, idx=idx, second_gap=second_gap, ties=int(np.count_nonzero(keys[1:] == keys[:-1])),
                abs_wx=np.abs(ew * X[idx]), abs_w=np.abs(ew), s_wx=s_wx, s_w=s_w)


def scale_vote(src, dst, nb, cbar2=1.0, block=None):
    """steps 1-2 -> dict(scale, scale_cost, n_pairs, n_degenerate_pairs, n_scale_inlier_pairs, pair_margin, vote (the
    tls_estimate dict over the pairs left), bound (relative bound of a reordered sum for the scale), X, r, degenerate)"""
    X, r, i, j, deg = pair_measurements(src, dst, nb, cbar2)
    keep = ~deg
    if not keep.any():
        return dict(valid=False, n_pairs=int(X.size), n_degenerate_pairs=int(deg.sum()))
    v = tls_estimate(X[keep], r[keep], block)
    s = v["estimate"]
    inl = np.abs(X[keep] - s) <= r[keep]
    margin = np.abs(np.abs(X[keep] - s) - r[keep]) / r[keep]
    k = v["min_index"]
    n_end = 2 * int(keep.sum())
    bound = 4 * n_end * U * (v["abs_wx"][:k + 1].sum() / abs(v["s_wx"][k]) + v["abs_w"][:k + 1].sum() / abs(v["s_w"][k]))
    return dict(valid=True, scale=s, scale_cost=v["cost"], n_pairs=int(X.size), n_degenerate_pairs=int(deg.sum()),
                n_scale_inlier_pairs=int(inl.sum()), pair_margin=float(margin.min()), vote=v, bound=float(bound), X=X, r=r,
                degenerate=deg)


def svd_rot(Xs, Ys, W):
    """utils.h:121-136.  Xs, Ys [n, 3], W [n] -> R [3, 3], the singular values of H"""
    H = (Xs * W[:, None]).T @ Ys
    Um, S, Vt = np.linalg.svd(H)
    V = Vt.T
    if np.linalg.det(Um) * np.linalg.det(V) < 0:
        V = V.copy(); V[:, 2] *= -1
    return V @ Um.T, S


def finish(src, dst, nb, scale, params):
    """registration.cc:594-690 for the chain graph, from the scale on -> dict(R, t, inliers, translation_mask, rotation_mask,
    rotation_iterations, weights, margins: dict of the smallest relative margins of the discrete decisions)"""
    src = np.asarray(src, np.float64); dst = np.asarray(dst, np.float64); nb = np.asarray(nb, np.float64)
    n = src.shape[0]
    leaf = np.concatenate([np.arange(1, n), [0]])
    ts = src[leaf] - src
    td = (dst[leaf] - dst) * (1 / scale)
    tb = (nb[leaf] + nb) * (1 / scale)
    bsq = tb * tb
    nbsq = (params["noise_bound"] * (2 / scale)) ** 2
    if nbsq < 1e-16:
        nbsq = 1e-2
    weights = np.ones(n)
    mu, prev_cost = 1.0, np.inf
    R = np.eye(3)
    thr = params["rotation_cost_threshold"]
    m_cost, m_mu, sing = np.inf, np.inf, None
    it = 0
    while it < params["rotation_max_iterations"]:
        R, sing = svd_rot(ts, td, weights)
        res = td - ts @ R.T
        rsq = (res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + res[:, 2] * res[:, 2]
        if it == 0:
            q = 2 * rsq.max() / nbsq - 1
            m_mu = abs(q)
            mu = 1 / q if q != 0 else np.inf
            if mu <= 0:
                break
        th1 = (mu + 1) / mu * bsq
        th2 = mu / (mu + 1) * bsq
        cost = float(np.cumsum(weights * rsq)[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(bsq * mu * (mu + 1) / rsq) - mu
        weights = np.where(rsq >= th1, 0.0, np.where(rsq <= th2, 1.0, mid))
        cost_diff = abs(cost - prev_cost)
        mu *= params["rotation_gnc_factor"]
        prev_cost = cost
        if np.isfinite(cost_diff):
            m_cost = min(m_cost, abs(cost_diff - thr) / thr)
        if cost_diff < thr:
            break
        it += 1
    rot_mask = weights >= 0.5
    alphas = nb * np.sqrt(params["cbar2"])
    raw = dst - scale * (src @ R.T)
    t = np.zeros(3)
    mask = np.ones(n, bool)
    m_t, m_gap = np.inf, np.inf
    for a in range(3):
        v = tls_estimate(raw[:, a], alphas)
        t[a] = v["estimate"]
        mask &= v["inliers"]
        m_t = min(m_t, float((np.abs(np.abs(raw[:, a] - t[a]) - alphas) / alphas).min()))
        m_gap = min(m_gap, v["second_gap"] / max(abs(v["cost"]), 1e-300))
    sum_ab = float((np.linalg.norm(ts, axis=1) * np.linalg.norm(td, axis=1)).sum())
    return dict(R=R, t=t, inliers=np.nonzero(mask)[0].astype(np.int32), translation_mask=mask, rotation_mask=rot_mask,
                rotation_iterations=it, weights=weights, singular_values=sing, sum_ab=sum_ab, raw_abs_max=float(np.abs(raw).max()),
                src_norm_max=float(np.linalg.norm(src, axis=1).max()), rotation_cost=float(prev_cost),
                margins=dict(translation=m_t, translation_cost_gap=m_gap, weight=float(np.abs(weights - 0.5).min() / 0.5),
                             cost_diff=m_cost, mu=m_mu))


def solve(src, dst, nb, params, block=None):
    """the whole solve -> the vote's dict and the finish's, merged (valid False: no pair was left in the vote)"""
    src = np.asarray(src); dst = np.asarray(dst); nb = np.asarray(nb)
    v = scale_vote(src, dst, nb, params["cbar2"], block)
    if not v["valid"]:
        return v
    f = finish(src, dst, nb, v["scale"], params)
    out = dict(v)
    out.update(f)
    out["n_inliers"] = int(f["inliers"].size)
    out["n_rotation_inliers"] = int(f["rotation_mask"].sum())
    return out


# the problems of tests/golden/registration_<name>.npz (tests/golden/make_registration_golden.py) and of the GPU tests:
# name -> arguments of synth.make_registration_problem.  "reference": the reference's solver wrote the expected results (it
# has no defined behaviour for coincident src points: that case is compared with this restatement alone)
CASES = {
    "n2": dict(N=2, seed=1, outlier_rate=0.0, noise=0.3, variant="plain", reference=True),
    "n3": dict(N=3, seed=1, outlier_rate=0.0, noise=0.3, variant="plain", reference=True),
    "n33": dict(N=33, seed=1, outlier_rate=0.3, noise=0.3, variant="plain", reference=True),
    "n64_o0": dict(N=64, seed=1, outlier_rate=0.0, noise=0.3, variant="plain", reference=True),
    "n64_o30": dict(N=64, seed=2, outlier_rate=0.3, noise=0.3, variant="plain", reference=True),
    "n64_o70": dict(N=64, seed=3, outlier_rate=0.7, noise=0.3, variant="plain", reference=True),
    "n64_all_outliers": dict(N=64, seed=4, outlier_rate=1.0, noise=0.3, variant="all_outliers", reference=True),
    "n64_noise_free": dict(N=64, seed=5, outlier_rate=0.0, noise=0.0, variant="noise_free", reference=True),
    "n64_coincident_dst": dict(N=64, seed=6, outlier_rate=0.3, noise=0.3, variant="coincident_dst", reference=True),
    "n64_coincident_src": dict(N=64, seed=7, outlier_rate=0.3, noise=0.3, variant="coincident_src", reference=False),
    "n64_clamp": dict(N=64, seed=8, outlier_rate=0.3, noise=0.3, variant="clamp", reference=True),
    "n257": dict(N=257, seed=1, outlier_rate=0.3, noise=0.3, variant="plain", reference=True),
    "n512_o50": dict(N=512, seed=1, outlier_rate=0.5, noise=0.3, variant="plain", reference=True),
    "n1024": dict(N=1024, seed=1, outlier_rate=0.3, noise=0.3, variant="plain", reference=True),
}


def make_case(name):
    from sage_slam_amd import synth
    kw = {k: v for k, v in CASES[name].items() if k != "reference"}
    return synth.make_registration_problem(**kw)


import functools
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> (fixture: dict of arrays, params: dict) of tests/golden/registration_<name>.npz"""
    with np.load(os.path.join(GOLDEN, "registration_%s.npz" % name)) as z:
        fx = {k: z[k] for k in z.files}
    params = dict(zip([str(s) for s in fx["params_names"]], [float(v) for v in fx["params_values"]]))
    for k in ("rotation_max_iterations", "rotation_tim_graph", "inlier_selection_mode", "rotation_algorithm"):
        params[k] = int(params[k])
    return fx, params


@functools.lru_cache(maxsize=None)
def restated(name):
    """the sequential restatement's solve of a fixture's problem, computed once per session"""
    fx, params = load_case(name)
    return solve(fx["src"], fx["dst"], fx["noise_bounds"], params)


def rotation_bound(sol, n):
    """Bound on |dR| between two fp64 evaluations of the finish that differ in summation order and SVD algorithm: per svdRot
    the sums of H carry at most (n + 16) u sum |a_i| |b_i| (n terms; 16 u |H| for the backward error of a 3x3 SVD), the polar
    factor moves by at most 2 |dH| / (sigma_2 - sigma_3) (the smaller of the two denominators, with and without the
    determinant fix), and the GNC feeds R back through continuous weights once per iteration: (iterations + 1) such steps, 8
    for the feedback."""
    S = sol["singular_values"]
    return 8 * (sol["rotation_iterations"] + 1) * (n + 16) * U * 2 * sol["sum_ab"] / max(S[1] - S[2], 1e-300)


def translation_bound(sol, n, d_rot, d_scale_rel):
    """... and on |dt|: a vote's estimate is a weighted mean of raw = dst - s R src over its consensus set, so it moves with
    the raw values (|s| |dR| |src| + |ds| |src|) and by the sum's own rounding, 4 n u max |raw|"""
    return sol["scale"] * (d_rot + d_scale_rel) * sol["src_norm_max"] * np.sqrt(3.0) + 4 * n * U * sol["raw_abs_max"]
