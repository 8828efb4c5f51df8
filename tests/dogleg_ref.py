"""fp64 numpy restatements for the dogleg tests: the dogleg point, gtsam's trust-region iteration in its three modes, and the
dense system A, g of a window as damped_system.h defines it at damping 0.

The point and the iteration are written from the vectors' side -- u, n and their norms, as DoglegOptimizerImpl.cpp:25-83 and
DoglegOptimizerImpl.h:137-252 state them -- with only the dot products as inputs, so that the engine's (a, b) form has
something independent to agree with."""
import numpy as np

SEARCH_EACH_ITERATION, SEARCH_REDUCE_ONLY, ONE_STEP_PER_ITERATION = 0, 1, 2
GG, GN, NN, GAG, GAN, NAN_ = range(6)


def dots_of(A, g, n):
    """the six dot products of a system"""
    Ag, An = A @ g, A @ n
    return np.array([g @ g, g @ n, n @ n, g @ Ag, g @ An, n @ An])


def point(delta, gg, gn, nn, gAg):
    """ComputeDoglegPoint / ComputeBlend -> (a, b, region) with the dogleg point = a g + b n; None for g.Ag <= 0"""
    if gg == 0.0:
        return 0.0, 0.0, 0
    if not gAg > 0.0:
        return None
    s = gg / gAg                                   # u = s g (optimizeGradientSearch)
    uu, un = s * s * gg, s * gn
    if delta * delta < uu:
        return np.sqrt(delta * delta / uu) * s, 0.0, 0
    if delta * delta < nn:
        qa, qb, qc = uu - 2.0 * un + nn, 2.0 * (un - uu), uu - delta * delta
        with np.errstate(invalid="ignore", divide="ignore"):
            root = np.sqrt(np.float64(qb * qb - 4.0 * qa * qc))
            t1, t2 = (-qb + root) / (2.0 * qa), (-qb - root) / (2.0 * qa)
        tau = t1 if 0.0 <= t1 <= 1.0 else t2
        return (1.0 - tau) * s, tau, 1
    return 0.0, 1.0, 2


def step_norm(d, a, b):
    return float(np.sqrt(a * a * d[GG] + 2 * a * b * d[GN] + b * b * d[NN]))


def model_decrease(d, a, b):
    """E(x) - E_model(x + delta) with E_model = E - 2 g.delta + delta.A delta"""
    return 2.0 * (a * d[GG] + b * d[GN]) - (a * a * d[GAG] + 2.0 * a * b * d[GAN] + b * b * d[NAN_])


def iterate(delta, mode, d, f_error, fn, min_delta=1e-5):
    """DoglegOptimizerImpl::Iterate around fn(a, b) -> error.  Returns dict(delta, rho, a, b, region, evals, accepted,
    candidate_error)."""
    a = b = 0.0
    region, evals, rho, f_cand = 0, 0, 0.5, f_error
    stay = d[GG] != 0.0
    last = None
    while stay:
        a, b, region = point(delta, d[GG], d[GN], d[NN], d[GAG])
        f_cand = float(fn(a, b))
        evals += 1
        f_dec, m_dec = f_error - f_cand, model_decrease(d, a, b)
        rho = 0.5 if abs(f_dec) < 1e-15 or abs(m_dec) < 1e-15 else f_dec / m_dec
        if rho >= 0.75:
            new = max(delta, 3.0 * step_norm(d, a, b))
            if mode != SEARCH_EACH_ITERATION:
                stay = False
            elif abs(new - delta) < 1e-15 or last == "decreased":
                stay = False
            else:
                last = "increased"
            delta = new
        elif rho >= 0.25:
            stay = False
        elif rho >= 0.0:
            hit = not delta > min_delta
            new = delta if hit else 0.5 * delta
            if mode == ONE_STEP_PER_ITERATION or last == "increased" or hit:
                stay = False
            else:
                last = "decreased"
            delta = new
        else:                                      # the error rose, or NaN
            if delta > min_delta:
                delta *= 0.5
                last = "decreased"
            else:
                a = b = 0.0
                f_cand = f_error
                stay = False
    return dict(delta=delta, rho=rho, a=a, b=b, region=region, evals=evals, accepted=int(a != 0.0 or b != 0.0),
                candidate_error=f_cand)


def row_held(mask, r, CS):
    return bool(mask & (1 if r < 6 else (2 if r < 6 + CS else 4)))


def dense_system(capi, packed, w_links, K, CS, dadd, gadd, holds=None):
    """A, g at damping 0: capi.unpack_dense (diagonal blocks as 0.5 (D + D^T)), the priors' diagonal and gradient
    (tests.helpers.prior_vectors), then the held rule: a held row / column is the identity's, its g entry 0 (no prior)."""
    B = 7 + CS
    H, g, _ = capi.unpack_dense(np.asarray(packed, np.float64), K, w_links, CS)
    A = H + np.diag(dadd)
    g = g + gadd
    held = np.zeros(K * B, bool)
    for k, mask in (holds or {}).items():
        for r in range(B):
            held[k * B + r] = row_held(mask, r, CS)
    A[held, :] = 0.0
    A[:, held] = 0.0
    A[held, held] = 1.0
    g[held] = 0.0
    return A, g, held
