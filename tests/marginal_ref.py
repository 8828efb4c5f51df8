"""fp64 numpy restatement of the marginal priors (include/sage_ba.h "f7"): the Schur complement, a prior's term at given
variables, where the term lands in the packed system, and the marginalisation of a window fed from its per-edge results.

Convention (the window's): e(d) = e - 2 g'd + d'Ad, step A d = g.  A prior over m keyframes is a dict(Lambda [mB,mB],
eta [mB], c, pose12 [m,12], code [m,CS], scale [m]); rows per keyframe: pose 6, code CS, scale 1.  Written from the header's
text; numpy's ``solve`` stands where the engine runs its Cholesky."""
from itertools import combinations

import numpy as np

from sage_slam_amd import capi as C

HOLD_POSE, HOLD_CODE, HOLD_SCALE = 1, 2, 4


# ------------------------------------------------------------------------------------------------ part 1: the marginal
def schur_marginal(A, g, e, drop):
    """(A, g, e) with the rows ``drop`` eliminated -> Lambda, eta, c over the other rows, ascending"""
    A = np.asarray(A, np.float64); g = np.asarray(g, np.float64)
    A = 0.5 * (A + A.T)
    d = np.asarray(drop, int).reshape(-1)
    k = np.setdiff1d(np.arange(g.size), d)
    if d.size == 0:
        return A[np.ix_(k, k)], g[k].copy(), float(e)
    X = np.linalg.solve(A[np.ix_(d, d)], np.column_stack([A[np.ix_(d, k)], g[d]]))
    S = A[np.ix_(k, k)] - A[np.ix_(k, d)] @ X[:, :-1]
    return 0.5 * (S + S.T), g[k] - A[np.ix_(k, d)] @ X[:, -1], float(e - g[d] @ X[:, -1])


def schur_bound(n, A_dd):
    """the textbook bound of a Cholesky solve in fp64, relative Frobenius norm: 64 n 2^-53 cond(A_dd)"""
    return 64.0 * n * 2.0 ** -53 * np.linalg.cond(A_dd)


def pose_local(origin12, other12):
    """[t1 - R1 R0' t0, log(R1 R0')] of two poses (R row-major, then t)"""
    o = np.asarray(origin12, np.float64); x = np.asarray(other12, np.float64)
    R0, t0, R1, t1 = o[:9].reshape(3, 3), o[9:], x[:9].reshape(3, 3), x[9:]
    Rr = R1 @ R0.T
    th = np.arccos(np.clip(0.5 * (np.trace(Rr) - 1.0), -1.0, 1.0))
    k = 0.5 if th < 1e-8 else th / (2.0 * np.sin(th))
    return np.concatenate([t1 - Rr @ t0, k * np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])])


def prior_delta(prior, pose12, code, scale):
    pose12 = np.asarray(pose12).reshape(-1, 12); code = np.asarray(code, np.float64).reshape(pose12.shape[0], -1)
    scale = np.asarray(scale, np.float64).reshape(-1)
    return np.concatenate([np.concatenate([pose_local(prior["pose12"][k], pose12[k]),
                                           code[k] - np.asarray(prior["code"][k], np.float64),
                                           [scale[k] - float(prior["scale"][k])]]) for k in range(pose12.shape[0])])


def prior_evaluate(prior, pose12, code, scale):
    """the term at the given variables of the prior's keyframes -> dict(delta, AtA, Atb, err)"""
    d = prior_delta(prior, pose12, code, scale)
    Lam, eta = np.asarray(prior["Lambda"]), np.asarray(prior["eta"])
    return dict(delta=d, AtA=Lam, Atb=eta - Lam @ d, err=float(d @ Lam @ d - 2.0 * eta @ d + prior["c"]))


def dot_bound(prior, delta, N):
    """componentwise bound of an N-term fp64 dot product on Atb_i = eta_i - (Lambda delta)_i: gamma_N (|eta| + |Lambda||delta|)_i,
    gamma_N = N 2^-53 / (1 - N 2^-53); and the same on err = delta'Lambda delta - 2 eta'delta + c"""
    gam = N * 2.0 ** -53 / (1.0 - N * 2.0 ** -53)
    Lam, eta, d = np.abs(prior["Lambda"]), np.abs(prior["eta"]), np.abs(delta)
    return gam * (eta + Lam @ d), gam * (d @ Lam @ d + 2.0 * eta @ d + abs(prior["c"]))


# ------------------------------------------------------------------------------------------------ part 3: the layout
def missing_links(links, kf_map):
    """the structure-only links a term appends: the pairs of its keyframes without a link, ascending (a, b)"""
    have = {(min(a, b), max(a, b)) for a, b in links}
    return sorted({(min(a, b), max(a, b)) for a, b in combinations(list(kf_map), 2)} - have)


def place_prior(K, links, CS, kf_map, AtA, Atb, err, packed=None):
    """the term added to a packed system [K diag | link blocks | g | tail] (zeros when none is given): diagonal blocks,
    link blocks [row in the older keyframe][column in the newer] -- transposed where the prior orders the pair the other way
    round --, gradient rows, the error in the geometric slot.  Every pair must have a link (the first of duplicates takes it)"""
    B = 7 + CS
    BB = B * B
    nl = len(links)
    out = np.zeros((K + nl) * BB + K * B + 4) if packed is None else np.array(packed, np.float64)
    diag = out[:K * BB].reshape(K, B, B); lnk = out[K * BB:(K + nl) * BB].reshape(nl, B, B)
    g = out[(K + nl) * BB:(K + nl) * BB + K * B].reshape(K, B)
    lk = [(min(a, b), max(a, b)) for a, b in links]
    AtA = np.asarray(AtA); Atb = np.asarray(Atb)
    for i, ki in enumerate(kf_map):
        diag[ki] += AtA[i * B:(i + 1) * B, i * B:(i + 1) * B]
        g[ki] += Atb[i * B:(i + 1) * B]
        for j in range(i + 1, len(kf_map)):
            kj = kf_map[j]
            blk = AtA[i * B:(i + 1) * B, j * B:(j + 1) * B]
            lnk[lk.index((min(ki, kj), max(ki, kj)))] += blk if ki < kj else blk.T
    out[-3] += err
    return out


# ------------------------------------------------------------------------------------------------ part 2: marginalize
def prior_rows(K, CS, poses, codes, scales, code_w, scale_w=0.0, pose_w=0.0, pose_init0=None, scale_init0=None, hold=None):
    """the window's own diagonal priors at the given variables (damped_system.h: prior_row) -> dadd, gadd [K, B] and each
    keyframe's share of the total error as sage_window_total_error counts it [K]"""
    B = 7 + CS
    dadd = np.zeros((K, B)); gadd = np.zeros((K, B)); err = np.zeros(K)
    for k in range(K):
        c = np.asarray(codes[k], np.float64)
        dadd[k, 6:6 + CS] = code_w; gadd[k, 6:6 + CS] = -code_w * c
        err[k] = code_w * float(c @ c) / CS
        if k == 0 and scale_w > 0:
            s = float(scales[0])
            dadd[0, 6 + CS] = scale_w / (s * s)
            gadd[0, 6 + CS] = scale_w / s * (np.log(float(scale_init0)) - np.log(s))
            err[0] += scale_w * (np.log(float(scale_init0)) - np.log(s)) ** 2
        if k == 0 and pose_w > 0:
            loc = pose_local(poses[0], pose_init0)
            dadd[0, :6] = pose_w; gadd[0, :6] = pose_w * loc
            err[0] += pose_w * float(loc @ loc)
        if hold and hold.get(k, 0):
            m = held_rows(hold[k], CS)
            dadd[k, m] = 0.0; gadd[k, m] = 0.0
    return dadd, gadd, err


def held_rows(mask, CS):
    m = np.zeros(7 + CS, bool)
    m[:6] = bool(mask & HOLD_POSE); m[6:6 + CS] = bool(mask & HOLD_CODE); m[6 + CS] = bool(mask & HOLD_SCALE)
    return m


def separator(K, links, drop, prior_maps=()):
    """every surviving keyframe that shares a link or a prior term with a dropped one, ascending"""
    drop = set(drop); sep = set()
    for a, b in links:
        if (a in drop) != (b in drop):
            sep.add(b if a in drop else a)
    for km in prior_maps:
        if drop & set(km):
            sep |= set(km) - drop
    return sorted(sep)


def marginalize(K, links, CS, edge_results, drop, dadd=None, gadd=None, prior_err=None, priors=(), hold=None, info=None):
    """the prior the keyframes ``drop`` leave behind, from the window's per-edge results.
    ``edge_results``: as ``capi.assemble_packed`` takes them -- every factor of the window; only those incident to a dropped
    keyframe are summed.  ``dadd, gadd, prior_err``: ``prior_rows``; ``priors``: [(term dict of ``prior_evaluate`` at the
    window's variables, kf_map)]; ``info``: a dict that receives n, the sub-system's rows, and bound = ``schur_bound``.
    -> Lambda, eta, c, separator"""
    B = 7 + CS
    drop = sorted(int(k) for k in drop)
    inc = {key: r for key, r in edge_results.items() if set(links[key[1]]) & set(drop)}
    packed = C.assemble_packed(K, links, CS, inc)
    e = float(packed[-4] + packed[-3])
    prior_maps = [km for _t, km in priors]
    for t, km in priors:
        if set(km) & set(drop):
            packed = place_prior(K, links, CS, km, t["AtA"], t["Atb"], 0.0, packed)
            e += t["err"]
    H, g, _tail = C.unpack_dense(packed, K, links, CS)
    for k in drop:
        if dadd is not None:
            H[k * B:(k + 1) * B, k * B:(k + 1) * B] += np.diag(dadd[k]); g[k * B:(k + 1) * B] += gadd[k]
            e += float(prior_err[k])
    sep = separator(K, links, drop, prior_maps)
    for k in drop + sep:                        # the hold rule: identity rows on dropped keyframes, zero rows on the separator
        if hold and hold.get(k, 0):
            rows = k * B + np.nonzero(held_rows(hold[k], CS))[0]
            H[rows, :] = 0.0; H[:, rows] = 0.0; g[rows] = 0.0
            if k in drop:
                H[rows, rows] = 1.0
    order = drop + sep
    idx = np.concatenate([np.arange(k * B, (k + 1) * B) for k in order])
    nd = len(drop) * B
    if info is not None:
        info.update(n=idx.size, bound=schur_bound(idx.size, H[np.ix_(idx[:nd], idx[:nd])]))
    Lam, eta, c = schur_marginal(H[np.ix_(idx, idx)], g[idx], e, np.arange(nd))
    return Lam, eta, c, sep


def dense_system(packed, K, links, CS, dadd, gadd, hold=None):
    """H, g of a packed system with the window's diagonal priors and the hold rule: what a damp-0 solve solves"""
    B = 7 + CS
    H, g, _ = C.unpack_dense(np.asarray(packed, np.float64), K, links, CS)
    H = H + np.diag(np.asarray(dadd).reshape(-1)); g = g + np.asarray(gadd).reshape(-1)
    for k in range(K):
        if hold and hold.get(k, 0):
            rows = k * B + np.nonzero(held_rows(hold[k], CS))[0]
            H[rows, :] = 0.0; H[:, rows] = 0.0; g[rows] = 0.0; H[rows, rows] = 1.0
    return H, g
