"""Marginal priors on the GPU (include/sage_ba.h "f7"): the prior term of a window (prior_eval_kernel, prior_add_kernel) and
sage_window_marginalize, against sage_prior_evaluate and the fp64 restatement of tests/marginal_ref.py.

Windows: synth.make_window(K, H=24, W=32, FS=16, L=2, n_samples=300, back_links=3), CS = 16 and 32 -> B = 23 and 39; priors
over 3 and 4 keyframes have 69 and 156 rows, ragged against the evaluation kernel's 64-row tile.

Bars.
* The term: Atb_i = eta_i - (Lambda delta)_i is an N-term fp64 dot product, N = mB + 16 (16 for the device's acos / sin against
  the host's); each side lies within gamma_N (|eta| + |Lambda||delta|)_i of the exact value, gamma_N = N 2^-53 / (1 - N 2^-53).
  The same for err = delta'Lambda delta - 2 eta'delta + c with |delta|'|Lambda||delta| + 2|eta|'|delta| + |c|.
  AtA is Lambda bit for bit; Lambda reaches the packed blocks as fl(assembled + image), checked bit for bit.
* The marginal: 64 n 2^-53 cond(A_dd), n the rows of the sub-system, relative Frobenius norm (marginal_ref.schur_bound).
* Steps: the project's LM-delta bar, rel-L2 <= 1e-4.

Measured on an MI355X (summary_line prints the figures on every run; DESIGN.md s3 "Marginal priors" quotes them): the term
within 0.05 (Atb) / 0.013 (err) of its bound at 23, 69 and 156 rows; marginalise {0} of K = 7 (CS 16): Lambda / eta / c
1.0e-11 / 1.9e-11 / 1.2e-11 against the restatement (bar 1.3e-4: cond(A_dd) ~ 1e8 on these scenes), the next window's damp-0
step against the full window's 6.9e-5; {0, 1} of K = 6 (CS 32): 4.4e-12 / 9.1e-12 / 1.1e-12, step 3.4e-5 -- the step's
distance is the fp32 rounding of the per-edge results the marginal is summed from (the packed buffer is assembled from their
unrounded doubles) times the undamped system's conditioning.  Chained {0} then {1} against {0, 1}: 2.8e-15 / 4.7e-7 / 4.8e-7
(pose_local(x, x) is not exactly zero).  LM / dogleg step with a prior against numpy: 3.0e-8 / 1.5e-8.  Sharded: rank 0 + rank 1
against the single rank 1.1e-16."""
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import marginal_ref as M
from tests.conftest import summary_line
from tests.helpers import rel
from tests.test_marginal_host import random_spd

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOT_PSD, STATE = -1, -2, -3, -4
CODE_W, SCALE_W, POSE_W = 1.0e-3, 1.0e4, 1.0e4           # capi.Window's defaults
TOL_DELTA = 1e-4
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


# ------------------------------------------------------------------------------------------------------------- scenes
def scene(K, CS, extra=()):
    w = synth.make_window(K=K, H=24, W=32, FS=16, CS=CS, L=2, n_samples=300, seed=41, back_links=3)
    return dataclasses.replace(w, links=list(w.links) + [lk for lk in extra if lk not in w.links])


def sub_scene(w, keep):
    """the keyframes ``keep`` of w with the links among them, renumbered"""
    pos = {k: i for i, k in enumerate(keep)}
    return dataclasses.replace(w, keyframes=[w.keyframes[k] for k in keep],
                               links=[(pos[a], pos[b]) for a, b in w.links if a in pos and b in pos])


def variables(win):
    v = [win.get_keyframe(k) for k in range(win.K)]
    return (np.array([p for p, _c, _s in v]), np.array([c for _p, c, _s in v]), np.array([s for _p, _c, s in v], np.float32))


def perturb(capi, win, seed, angle=0.05):
    """move every keyframe: a rotation of about ``angle`` rad, a few percent of translation, code and scale"""
    rng = np.random.default_rng(seed)
    for k in range(win.K):
        p, c, s = win.get_keyframe(k)
        w3 = rng.normal(size=3); w3 *= angle * rng.uniform(0.5, 2.0) / np.linalg.norm(w3)
        win.set_keyframe(k, capi.pose_retract(p, np.concatenate([rng.normal(0, 0.01, 3), w3])),
                         c + rng.normal(0, 0.01, c.size).astype(np.float32), float(np.float32(s * np.exp(rng.normal(0, 0.01)))))


def random_prior(capi, win, kf_map, seed, scale=50.0):
    """a prior linearised at the window's current variables of ``kf_map``: Lambda SPD with cond 1e3, eta, c"""
    rng = np.random.default_rng(seed)
    pose, code, scl = variables(win)
    n = len(kf_map) * win.B
    Lam = scale * random_spd(rng, n, 1e3)
    d = dict(Lambda=0.5 * (Lam + Lam.T), eta=rng.normal(size=n), c=float(rng.uniform(0.5, 2.0)), pose12=pose[kf_map],
             code=code[kf_map], scale=scl[kf_map])
    return capi.MarginalPrior(keyframes=kf_map, **d), d


def edge_results(win, w):
    return {(t, l, d): win.get_edge(t, 2 * l + d) for t in (0, 1) for l in range(len(w.links)) for d in (0, 1)}


def window_priors(w, win, code_w=CODE_W, scale_w=SCALE_W, pose_w=POSE_W, hold=None):
    """dadd, gadd, per-keyframe error of the window's diagonal priors at its current variables"""
    pose, code, scl = variables(win)
    kf0 = w.keyframes[0]
    return M.prior_rows(win.K, w.CS, pose, code, scl, code_w, scale_w, pose_w,
                        pose_init0=np.concatenate([kf0.R.ravel(), kf0.t]).astype(np.float32), scale_init0=np.float32(kf0.scale), hold=hold)


def term_bounds(d, delta):
    N = delta.size + 16
    return M.dot_bound(d, delta, N)


# --------------------------------------------------------------------------------------------------- 1. the term alone
@pytest.mark.parametrize("CS,kf_map", [(16, [0, 1, 2]), (32, [3, 0, 2, 1]), (16, [2])])
def test_term_alone(capi, CS, kf_map):
    w = scene(4, CS)
    base = capi.Window(w)
    P, d = random_prior(capi, base, kf_map, seed=CS + len(kf_map))
    base.close()
    win = capi.Window(w, prior_terms=[(P, kf_map)])
    P.close()                                              # the window holds a copy
    assert win.num_prior_terms() == 1
    assert win.get_prior_term(0, check=False)[0] == STATE  # nothing evaluated yet
    perturb(capi, win, seed=1, angle=0.2)
    win.linearize()
    got = win.get_prior_term(0)
    pose, code, scl = variables(win)
    P2 = capi.MarginalPrior(**d)
    host = P2.evaluate(pose[kf_map], code[kf_map], scl[kf_map])
    assert np.array_equal(got["AtA"], d["Lambda"])         # bit for bit
    bA, bE = term_bounds(d, host["delta"])
    wA = float(np.max(np.abs(got["Atb"] - host["Atb"]) / bA)); wE = abs(got["err"] - host["err"]) / bE
    summary_line(f"prior term m {len(kf_map)} CS {CS} ({len(kf_map) * (7 + CS)} rows): Atb {wA:.3f}, err {wE:.3f} of the "
                 f"N-term dot-product bound against sage_prior_evaluate")
    assert np.all(np.abs(got["Atb"] - host["Atb"]) <= 2.0 * bA) and abs(got["err"] - host["err"]) <= 2.0 * bE
    # a second linearize: the same bits
    packed = win.packed_host().copy()
    win.linearize()
    again = win.get_prior_term(0)
    assert np.array_equal(again["Atb"], got["Atb"]) and again["err"] == got["err"] and np.array_equal(win.packed_host(), packed)
    # the error pass at the candidate set (set_keyframe wrote both sets) gives the same error as the linearize there: next to a
    # window without the prior, whose dense totals are the same bits, both tails carry the same double on top
    plain = capi.Window(w)
    for k in range(win.K):
        plain.set_keyframe(k, *win.get_keyframe(k))
    plain.linearize(); plain.error(1); win.error(1)
    t_lin, p_lin = win.packed_host()[-4:], plain.packed_host()[-4:]
    t_err, p_err = win.error_tensor().cpu().numpy(), plain.error_tensor().cpu().numpy()
    assert t_lin[1] == p_lin[1] + got["err"] and t_err[1] == p_err[1] + got["err"]
    assert t_lin[0] == p_lin[0] and t_err[0] == p_err[0] and np.array_equal(t_lin[2:], p_lin[2:]) and np.array_equal(t_err[2:], p_err[2:])
    assert win.total_error(False) - plain.total_error(False) == pytest.approx(got["err"], rel=1e-9)
    win.close(); plain.close()


# ------------------------------------------------------------------------------------------- 2. into the packed buffer
CASES_2 = [
    ("m = 1, no link block", 16, [[3]], None),
    ("kf_map descending: transposed blocks", 16, [[4, 2, 1]], None),
    ("descending, B = 39, a pair without a link", 32, [[4, 0]], None),
    ("two priors sharing a keyframe", 16, [[0, 2], [2, 3, 1]], None),
    ("a prior on a held keyframe", 16, [[1, 2]], {1: 7, 3: 2}),
]


@pytest.mark.parametrize("name,CS,maps,holds", CASES_2, ids=[c[0] for c in CASES_2])
def test_into_the_packed_buffer(capi, name, CS, maps, holds):
    K = 5
    w = scene(K, CS)
    base = capi.Window(w)
    priors = [random_prior(capi, base, km, seed=10 + i) for i, km in enumerate(maps)]
    base.close()
    win = capi.Window(w, prior_terms=[(P, km) for (P, _d), km in zip(priors, maps)], holds=holds)
    extra = win.links[len(w.links):]
    want_extra, have = [], list(w.links)
    for km in maps:
        new = M.missing_links(have, km)
        want_extra += new; have += new
    assert extra == want_extra
    plain = capi.Window(w, keypoint_links=extra, holds=holds)          # the same structure, no prior
    assert plain.links == win.links and plain.packed_count == win.packed_count
    for x in (win, plain):
        perturb(capi, x, seed=2, angle=0.1)
    win.linearize(); plain.linearize()
    pa, pb = win.packed_host(), plain.packed_host()
    pose, code, scl = variables(win)
    B = win.B
    nb = (K + len(win.links)) * B * B
    image = np.zeros_like(pa); grad = np.zeros(K * B); gbar = np.zeros(K * B); err = 0.0; ebar = 0.0
    for (P, d), km in zip(priors, maps):                              # term-id order
        ref = M.prior_evaluate(d, pose[km], code[km], scl[km])
        image = M.place_prior(K, win.links, CS, km, d["Lambda"], np.zeros(len(km) * B), 0.0, image)
        bA, bE = term_bounds(d, ref["delta"])
        for i, k in enumerate(km):
            grad[k * B:(k + 1) * B] += ref["Atb"][i * B:(i + 1) * B]
            gbar[k * B:(k + 1) * B] += bA[i * B:(i + 1) * B] + 4 * EPS * np.abs(ref["Atb"][i * B:(i + 1) * B])
        err += ref["err"]; ebar += bE + 4 * EPS * abs(ref["err"])
    assert np.array_equal(pa[:nb], pb[:nb] + image[:nb])              # the blocks: exact
    ga, gb = pa[nb:nb + K * B], pb[nb:nb + K * B]
    hit = np.repeat(np.isin(np.arange(K), [k for km in maps for k in km]), B)
    gbar += 4 * EPS * np.abs(gb)
    assert np.all(np.abs(ga - (gb + grad)) <= gbar)
    assert np.array_equal(ga[~hit], gb[~hit])                         # other keyframes: untouched
    assert abs(pa[-3] - (pb[-3] + err)) <= ebar + 4 * EPS * abs(pb[-3])
    assert pa[-4] == pb[-4] and pa[-2] == pb[-2] and pa[-1] == pb[-1]
    if holds:                                                          # the solver applies the hold rule to the sum
        win.solve(1e-3)
        d = win.delta().reshape(K, B)
        assert not d[1].any() and not d[3, 6:6 + CS].any() and d[2].all()
    summary_line(f"prior into packed, {name}: blocks exact; gradient {np.max(np.abs(ga - (gb + grad)) / np.where(gbar > 0, gbar, 1)):.3f}, "
                 f"error slot {abs(pa[-3] - (pb[-3] + err)) / (ebar + 4 * EPS * abs(pb[-3])):.3f} of their bars")
    win.close(); plain.close()


# ----------------------------------------------------------------------------- 3. the property that defines the feature
def marginalize_both(capi, w, win, drop, priors=(), hold=None, **weights):
    """sage_window_marginalize and the restatement fed from get_edge -> (prior, its dict, ref Lambda, eta, c, sep, bound)"""
    dadd, gadd, perr = window_priors(w, win, hold=hold, **weights)
    info = {}
    LamR, etaR, cR, sep = M.marginalize(win.K, win.links, w.CS, edge_results(win, w), drop, dadd, gadd, perr, priors=priors,
                                        hold=hold, info=info)
    P = win.marginalize(drop)
    got = P.get()
    assert got["keyframes"].tolist() == sep
    return P, got, LamR, etaR, cR, sep, info["bound"]


@pytest.mark.parametrize("K,CS,drop,want_sep,want_links", [(7, 16, [0], [1, 2, 3, 6], [(1, 6), (2, 6)]),
                                                           (6, 32, [0, 1], [2, 3, 4, 5], [])])
def test_marginal_reproduces_the_full_solve(capi, K, CS, drop, want_sep, want_links):
    B = 7 + CS
    w = scene(K, CS, extra=[(0, K - 1)])
    win = capi.Window(w)
    assert win.marginalize(drop, check=False)[0] == STATE              # no linearization yet
    win.linearize()
    dadd, gadd, _perr = window_priors(w, win)
    full = capi.block_solve(win.packed_host(), K, win.links, B, 0.0, dadd, gadd).reshape(K, B)
    P, got, LamR, etaR, cR, sep, bound = marginalize_both(capi, w, win, drop)
    assert sep == want_sep
    dL, de, dc = rel(got["Lambda"], LamR), rel(got["eta"], etaR), abs(got["c"] - cR) / abs(cR)
    assert dL <= bound and de <= bound and dc <= bound
    assert np.array_equal(got["Lambda"], got["Lambda"].T)
    pose, code, scl = variables(win)
    assert np.array_equal(got["pose12"], pose[sep]) and np.array_equal(got["code"], code[sep]) and np.array_equal(got["scale"], scl[sep])
    # the next window: the survivors with the same links and the prior; keyframe 0's pose and scale priors went into the marginal
    keep = [k for k in range(K) if k not in drop]
    w2 = sub_scene(w, keep)
    kf_map = [keep.index(k) for k in sep]
    win2 = capi.Window(w2, prior_terms=[(P, kf_map)], scale_prior_weight=0.0, pose_prior_weight=0.0)
    assert [(keep[a], keep[b]) for a, b in win2.links[len(w2.links):]] == want_links
    win2.linearize()
    win2.solve(0.0)
    d2 = win2.delta().reshape(len(keep), B)
    dist = rel(d2, full[keep])
    summary_line(f"marginalize {drop} of K {K} CS {CS}: separator {sep}; Lambda {dL:.2e}, eta {de:.2e}, c {dc:.2e} against the "
                 f"restatement (bar {bound:.2e}); damp-0 step of the next window vs the full window's {dist:.2e} (bar {TOL_DELTA})")
    assert dist <= TOL_DELTA
    win.close(); win2.close()


# ------------------------------------------------------------------------------------------ 4. chaining on the device
def test_chained_marginalisation(capi):
    K, CS = 6, 16
    B = 7 + CS
    w = scene(K, CS, extra=[(0, K - 1)])
    win = capi.Window(w)
    win.linearize()
    P01, got01, _L, _e, _c, sep01, bound = marginalize_both(capi, w, win, [0, 1])
    P0 = win.marginalize([0])
    sep0 = P0.get()["keyframes"].tolist()
    keep = list(range(1, K))
    w2 = sub_scene(w, keep)
    win2 = capi.Window(w2, prior_terms=[(P0, [keep.index(k) for k in sep0])], scale_prior_weight=0.0, pose_prior_weight=0.0)
    win2.linearize()                                                   # the same variables: the same per-edge results
    P1 = win2.marginalize([0])                                         # keyframe 1 of the first window
    got1 = P1.get()
    assert [keep[k] for k in got1["keyframes"]] == sep01
    dL, de, dc = rel(got1["Lambda"], got01["Lambda"]), rel(got1["eta"], got01["eta"]), abs(got1["c"] - got01["c"]) / abs(got01["c"])
    summary_line(f"chained marginalisation {{0}} then {{1}} vs {{0, 1}} at once: Lambda {dL:.2e}, eta {de:.2e}, c {dc:.2e} (bar {bound:.2e})")
    assert dL <= bound and de <= bound and dc <= bound
    win.close(); win2.close()


# -------------------------------------------------------------------------------------- 5. an LM step and a dogleg step
def next_window(capi, K=6, CS=16):
    """the window after {0} left a K + 1 window: (scene, kf_map, prior dict), perturbed variables applied by the caller"""
    w = scene(K + 1, CS, extra=[(0, K)])
    win = capi.Window(w)
    win.linearize()
    P = win.marginalize([0])
    d = P.get()
    keep = list(range(1, K + 1))
    win.close()
    return sub_scene(w, keep), [keep.index(k) for k in d["keyframes"]], d


def reference_system(capi, w2, kf_map, d, links, seed, damp):
    """(H, g) of assembled + prior + the window's code priors at the perturbed variables, from a window without the prior"""
    plain = capi.Window(w2, keypoint_links=links[len(w2.links):], scale_prior_weight=0.0, pose_prior_weight=0.0)
    perturb(capi, plain, seed=seed, angle=0.02)
    pose, code, scl = variables(plain)
    # the MERGED linearize of sage_window_lm_step / _dogleg_step (its fp32 sums differ from sage_window_linearize's by ~2e-6):
    # a classic LM step leaves the system of its linearisation point in the packed buffer
    cfg = capi.lm_config_default(); cfg.max_inner_evals = 1
    plain.lm_step(capi.SageLmState(), cfg)
    ref = M.prior_evaluate(d, pose[kf_map], code[kf_map], scl[kf_map])
    packed = M.place_prior(plain.K, links, w2.CS, kf_map, ref["AtA"], ref["Atb"], ref["err"], plain.packed_host())
    dadd, gadd, perr = M.prior_rows(plain.K, w2.CS, pose, code, scl, CODE_W)
    H, g = M.dense_system(packed, plain.K, links, w2.CS, dadd, gadd)
    return plain, H, g, float(packed[-4] + packed[-3] + perr.sum())


def host_error(capi, plain, d, kf_map, cand):
    """the total error at the variables ``cand``: the window without the prior + sage_prior_evaluate"""
    for k, v in enumerate(cand):
        plain.set_keyframe(k, *v)
    plain.error(1)
    pose, code, scl = variables(plain)
    P = capi.MarginalPrior(**{k: d[k] for k in ("Lambda", "eta", "c", "pose12", "code", "scale")})
    ev = P.evaluate(pose[kf_map], code[kf_map], scl[kf_map])
    return plain.total_error(False) + ev["err"], term_bounds(d, ev["delta"])[1]


def test_lm_step_with_a_prior(capi):
    w2, kf_map, d = next_window(capi)
    P = capi.MarginalPrior(**{k: d[k] for k in ("Lambda", "eta", "c", "pose12", "code", "scale")})
    win = capi.Window(w2, prior_terms=[(P, kf_map)], scale_prior_weight=0.0, pose_prior_weight=0.0)
    perturb(capi, win, seed=5, angle=0.02)
    damp = 1e-3
    plain, H, g, e_ref = reference_system(capi, w2, kf_map, d, win.links, 5, damp)
    cfg = capi.lm_config_default(); cfg.init_damp = damp; cfg.max_inner_evals = 1
    st = capi.SageLmState()
    win.lm_step(st, cfg)
    want = np.linalg.solve(H + damp * np.diag(np.diag(H)), g)
    dist = rel(win.delta(), want)
    assert dist <= TOL_DELTA
    assert st.error == pytest.approx(e_ref, rel=2e-5)
    cand = [win.get_keyframe(k) for k in range(win.K)] if st.accepted else None
    assert st.accepted == int(st.candidate_error < st.error)
    assert st.accepted == 1
    e_host, bE = host_error(capi, plain, d, kf_map, cand)
    summary_line(f"LM step with a prior: delta vs numpy {dist:.2e}; error {st.error:.6f} -> {st.candidate_error:.6f}, host "
                 f"evaluation of the candidate {e_host:.6f}")
    assert abs(st.candidate_error - e_host) <= 2.0 * bE + 8 * EPS * abs(e_host)
    win.close(); plain.close()


def test_dogleg_step_with_a_prior(capi):
    w2, kf_map, d = next_window(capi)
    P = capi.MarginalPrior(**{k: d[k] for k in ("Lambda", "eta", "c", "pose12", "code", "scale")})
    win = capi.Window(w2, prior_terms=[(P, kf_map)], scale_prior_weight=0.0, pose_prior_weight=0.0)
    perturb(capi, win, seed=6, angle=0.02)
    plain, H, g, e_ref = reference_system(capi, w2, kf_map, d, win.links, 6, 0.0)
    n = np.linalg.solve(H, g)
    cfg = capi.dogleg_config_default(); cfg.init_delta = 0.5 * float(np.linalg.norm(n))    # inside the Gauss-Newton point
    cfg.mode = capi.SAGE_DOGLEG_ONE_STEP_PER_ITERATION
    st = capi.SageDoglegState()
    win.dogleg_step(st, cfg)
    from tests import dogleg_ref as D
    a, b, region = D.point(cfg.init_delta, g @ g, g @ n, n @ n, g @ H @ g)
    want = a * g + b * n
    dist = rel(win.delta(), want)
    assert (st.region, st.evals) == (region, 1) and dist <= TOL_DELTA
    assert st.error == pytest.approx(e_ref, rel=2e-5)
    assert st.accepted == int(st.candidate_error < st.error) == 1
    e_host, bE = host_error(capi, plain, d, kf_map, [win.get_keyframe(k) for k in range(win.K)])
    summary_line(f"dogleg step with a prior: region {region}, step vs numpy {dist:.2e}; error {st.error:.6f} -> "
                 f"{st.candidate_error:.6f}, host evaluation {e_host:.6f}")
    assert abs(st.candidate_error - e_host) <= 2.0 * bE + 8 * EPS * abs(e_host)
    win.close(); plain.close()


# ------------------------------------------------------------------------------------------------------- 6. sharding
def test_sharded_windows_give_the_prior_to_rank_0(capi):
    K, CS = 5, 16
    w = scene(K, CS)
    base = capi.Window(w)
    P, d = random_prior(capi, base, [3, 0, 1], seed=3)
    base.close()
    packed = {}
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        win = capi.Window(w, rank=rank, world=world, prior_terms=[(P, [3, 0, 1])])
        plain = capi.Window(w, rank=rank, world=world, keypoint_links=win.links[len(w.links):])
        for x in (win, plain):
            perturb(capi, x, seed=4)
            x.linearize()
        packed[(rank, world)] = (win.packed_host().copy(), plain.packed_host().copy())
        assert win.get_prior_term(0, check=False)[0] == (0 if rank == 0 else INVALID)
        if world > 1:
            assert win.marginalize([0], check=False)[0] == UNSUPPORTED
        win.close(); plain.close()
    whole, r0, r1 = packed[(0, 1)], packed[(0, 2)], packed[(1, 2)]
    assert np.array_equal(r1[0], r1[1])                                # rank 1 carries nothing of the prior
    assert not np.array_equal(r0[0], r0[1])
    assert np.array_equal(r0[0] - r0[1] != 0, whole[0] - whole[1] != 0)
    dist = rel(r0[0] + r1[0], whole[0])
    summary_line(f"prior on a sharded window: rank 0 + rank 1 vs the single rank {dist:.2e}")
    assert dist <= 1e-12


# --------------------------------------------------------------------------------------------------------- 7. misuse
def test_misuse_answers_status_codes(capi):
    K, CS = 4, 16
    w = scene(K, CS)
    win = capi.Window(w)
    P, d = random_prior(capi, win, [0, 1], seed=1)
    P32 = capi.MarginalPrior(Lambda=np.eye(39), eta=np.zeros(39), c=0.0, pose12=np.zeros((1, 12)), code=np.zeros((1, 32)), scale=np.ones(1))
    L = capi.lib()
    # finalized: no more terms; nothing to get
    assert win.add_prior_term(P, [0, 1]) == STATE
    assert win.num_prior_terms() == 0 and L.sage_window_num_prior_terms(None) == 0
    assert win.get_prior_term(0, check=False)[0] == INVALID
    # marginalize: state, arguments
    assert win.marginalize([0], check=False)[0] == STATE               # no linearization
    win.linearize()
    for bad in ([K], [-1], [0, 0], list(range(K))):
        assert win.marginalize(bad, check=False)[0] == INVALID
    f = L.sage_window_marginalize
    h = capi.C.c_void_p()
    ids = np.zeros(1, np.int32)
    assert f(None, ids.ctypes.data, 1, capi.C.addressof(h)) == INVALID
    assert f(win.h, None, 1, capi.C.addressof(h)) == INVALID
    assert f(win.h, ids.ctypes.data, 0, capi.C.addressof(h)) == INVALID
    assert f(win.h, ids.ctypes.data, 1, None) == INVALID
    ok = win.marginalize([0])
    ok.close()
    p, c, s = win.get_keyframe(1)
    win.set_keyframe(1, p, c, s)                                       # new variables: the linearization is stale
    assert win.marginalize([0], check=False)[0] == STATE
    win.linearize()
    win.set_runs(2)                                                    # as sage_window_solve after sage_window_set_runs
    assert win.marginalize([0], check=False)[0] == STATE
    win.close()
    # before finalize: arguments (a window the constructor has not finalized yet: built by hand from its handle)
    fresh = capi.Window.__new__(capi.Window)
    cfgwin = capi.Window(w)
    fresh.h = capi.C.c_void_p()
    assert L.sage_window_create(capi.C.byref(cfgwin.cfg), None, capi.C.byref(fresh.h)) == 0
    fresh.win, fresh.links, fresh.prior_terms = w, [], []
    for k, (kf, dk) in enumerate(zip(w.keyframes, cfgwin.kfs)):
        v = dk.view()
        pose = capi.pack_pose(kf.R, kf.t); code = np.ascontiguousarray(kf.code, np.float32)
        assert L.sage_window_add_keyframe(fresh.h, capi.C.byref(v), capi._fp(pose), capi._fp(code), capi.C.c_float(kf.scale)) == k
    assert fresh.add_prior_term(None, [0, 1]) == INVALID
    assert fresh.add_prior_term(P, None) == INVALID
    assert fresh.add_prior_term(P, [0, 0]) == INVALID                  # duplicate
    assert fresh.add_prior_term(P, [0, K]) == INVALID                  # not a keyframe
    assert fresh.add_prior_term(P32, [0]) == INVALID                   # another code size
    assert L.sage_window_num_links(fresh.h) == 0                       # a refused call appends nothing
    assert fresh.add_prior_term(P, [2, 0]) == 0 and L.sage_window_num_links(fresh.h) == 1 and fresh.links == [(0, 2)]
    assert fresh.num_prior_terms() == 1
    assert fresh.get_prior_term(0, check=False)[0] == STATE            # not finalized
    assert fresh.marginalize([0], check=False)[0] == STATE
    L.sage_window_destroy(fresh.h); fresh.h = None
    cfgwin.close()
    # a separator above the cap: keyframe 0 linked to 17 others
    big = scene(18, CS)
    big = dataclasses.replace(big, links=list(big.links) + [(0, k) for k in range(4, 18)])
    bw = capi.Window(big)
    bw.linearize()
    assert bw.marginalize([0], check=False)[0] == UNSUPPORTED
    bw.close()
