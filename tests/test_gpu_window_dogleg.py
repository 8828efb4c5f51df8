"""The dogleg step on the GPU: the product kernels, the candidate kernel and a step replayed against fp64 numpy.

The windows are test_gpu_window_candidate.py's: 24 x 32 images, two levels, 300 samples.  1. to 3. hand the kernels an injected
well-conditioned system (that file's test 2: asymmetric diagonal storage, priors with a gradient), so the comparison runs at
the precision of the sums themselves; the dense A, g are tests/dogleg_ref.py's (unpack_dense + prior_vectors + the held rule).

1. products: Ag, An elementwise against numpy A @ (the device's g, n) within 2 (deg_k + 1) B eps (|A| |v|)_i -- a row of A has
   (deg_k + 1) B entries, summed in two stages; the six dots within 2 K B eps sum |x_i y_i|; n within the file's 64 eps cond(A);
   g against numpy's (see G_BAR); a second call in every bit.
2. the same with holds: held entries of g, Ag, n and delta exactly 0; compact solver rows.
3. candidate: delta elementwise within 4 eps (|a g_i| + |b n_i|) (two products and a sum, each rounded once; 4 leaves room for
   a fused and an unfused sum); (a, b) = (0, 1) leaves the bits of solve(0) alone.
4. five steps on a real window replayed: delta, rho, the new radius, the accepted variables; solves == iters.  A and g are
   rebuilt from the system the step leaves in `packed` (see the comment there: a linearize() at the same variables gives it to
   fp32 accuracy only, the step runs the merged linearize of the classic LM sequence).
5. sharded, reduced and duplicate-link windows refuse and keep working under lm_step.

Measured figures are printed through summary_line on every run."""
import dataclasses

import numpy as np
import pytest

from tests import dogleg_ref as ref
from tests.conftest import summary_line
from tests.helpers import prior_vectors, rel, retract_ref, retract_ref_f32
from tests.test_gpu_sharded_lm import _Recorder
from tests.test_gpu_window_candidate import (CODE_W, EPS32, EPS64, NOT_PSD, all_vars, inject, lost_scene, same_vars,
                                             small_window)

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
# g = packed gradient + the priors' gradients.  The code prior's is one product; keyframe 0's pose prior goes through
# acos((tr - 1) / 2) at an angle theta ~ 0.04, where the arccosine loses log2(1 / theta^2) ~ 9 bits -- in the engine's double
# code and in numpy alike -- and its scale prior through a difference of two logarithms 0.05 apart (4 to 5 bits).  Bar, per
# entry: 4 eps on the sum's terms, plus 2^10 eps on a pose / scale prior's gradient.
G_BAR_TERMS, G_BAR_PRIOR0 = 4 * EPS64, 2.0 ** 10 * EPS64


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


def general_window(capi, K, CS, extra, holds=None, seed=None):
    """test 2 of test_gpu_window_candidate.py: priors with a gradient on a keyframe 0 that has moved, a seeded system with
    asymmetric diagonal storage -> (window, synthetic window, A, g, held, gadd, packed g) with A, g the dense fp64 system"""
    B = 7 + CS
    w = small_window(K, CS, extra=extra)
    win = capi.Window(w, code_prior_weight=CODE_W, scale_prior_weight=10.0, pose_prior_weight=10.0, holds=holds)
    p0, c0, s0 = win.get_keyframe(0)
    win.set_keyframe(0, retract_ref_f32(p0, [0.01, -0.02, 0.015, 0.02, 0.01, -0.03]), c0, float(np.float32(1.05 * s0)))
    cur = all_vars(win)
    rng = np.random.default_rng((100 + K) if seed is None else seed)
    diag = np.stack([np.diag(1.0 + rng.uniform(0, 1, B)) + 0.02 * rng.standard_normal((B, B)) for _ in range(K)])
    assert not np.array_equal(diag[0], diag[0].T)
    packed = inject(win, diag, 0.02 * rng.standard_normal((len(w.links), B, B)), rng.standard_normal(K * B))
    dadd, gadd = prior_vectors(w, CS, code_w=CODE_W, codes=[c[1] for c in cur], pose0=cur[0][0], scale0=cur[0][2],
                               pose_w=10.0, scale_w=10.0)
    A, g, held = ref.dense_system(capi, packed, w.links, K, CS, dadd, gadd, holds)
    gp = packed[(K + len(w.links)) * B * B:(K + len(w.links)) * B * B + K * B]
    return win, w, A, g, held, np.where(held, 0.0, gadd), np.where(held, 0.0, gp)


def check_products(capi, name, win, w, A, g, held, gadd, gp):
    """solve(0), the products and every bar of 1.; returns (dots, g, Ag, n, An) of the device"""
    K, B, CS = win.K, win.B, w.CS
    deg = np.zeros(K, int)
    for a, b in w.links:
        deg[a] += 1
        deg[b] += 1
    cond = float(np.linalg.cond(A))
    assert cond < 100
    win.solve(0.0)
    dots = win.dogleg_products()
    gd, Agd, nd, And = win.dogleg_vectors()
    # g
    prior0 = np.zeros(K * B)
    prior0[:6] = np.abs(gadd[:6])
    prior0[6 + CS] = abs(gadd[6 + CS])
    g_bar = G_BAR_TERMS * (np.abs(gp) + np.abs(gadd)) + G_BAR_PRIOR0 * prior0
    g_worst = float(np.max(np.abs(gd - g) / np.where(g_bar > 0, g_bar, 1.0)))
    assert np.all(np.abs(gd - g) <= g_bar), (name, g_worst)
    # n
    d_n = rel(nd, np.linalg.solve(A, g))
    assert d_n <= 64 * EPS64 * cond
    assert np.array_equal(nd, win.delta())
    # Ag, An
    row_terms = np.repeat(2.0 * (deg + 1) * B * EPS64, B)
    worst = {}
    for tag, prod, v in (("Ag", Agd, gd), ("An", And, nd)):
        bar = row_terms * (np.abs(A) @ np.abs(v))
        err = np.abs(prod - A @ v)
        worst[tag] = float(np.max(err / np.where(bar > 0, bar, 1.0)))
        assert np.all(err <= bar), (name, tag, worst[tag])
    # the dots
    pairs = ((gd, gd), (gd, nd), (nd, nd), (gd, Agd), (gd, And), (nd, And))
    d_worst = 0.0
    for got, (x, y) in zip(dots, pairs):
        bar = 2.0 * K * B * EPS64 * float(np.sum(np.abs(x * y)))
        d_worst = max(d_worst, abs(got - float(x @ y)) / bar)
        assert abs(got - float(x @ y)) <= bar, (name, got, float(x @ y))
    # a second call: every bit
    dots2 = win.dogleg_products()
    again = win.dogleg_vectors()
    assert np.array_equal(dots, dots2) and all(np.array_equal(p, q) for p, q in zip((gd, Agd, nd, And), again))
    summary_line(f"dogleg products {name}: g {g_worst:.2f}, Ag {worst['Ag']:.2f}, An {worst['An']:.2f}, dots {d_worst:.3f} of "
                 f"their bars; n vs numpy {d_n:.2e} (cond {cond:.1f}, bar {64 * EPS64 * cond:.2e}); |An - g| / |g| "
                 f"{np.linalg.norm(And - gd) / np.linalg.norm(gd):.2e}; max degree {deg.max()}")
    return dots, gd, Agd, nd, And


# ------------------------------------------------------------------------------------------- 1. products on a general system
@pytest.mark.parametrize("K,CS,hub", [(18, 16, False), (6, 32, False), (12, 16, True)])
def test_products_on_an_injected_general_system(capi, K, CS, hub):
    """B = 23 and B = 39 with the loop link (0, K - 1); K = 12 with keyframe 0 linked to every other keyframe: its incidence
    list has twelve entries"""
    extra = [(0, k) for k in range(1, K)] if hub else [(0, K - 1)]
    win, w, A, g, held, gadd, gp = general_window(capi, K, CS, extra)
    if hub:
        assert sum(1 for a, b in w.links if 0 in (a, b)) == K - 1 > 6
    check_products(capi, f"K {K} CS {CS}" + (" hub" if hub else ""), win, w, A, g, held, gadd, gp)
    win.close()


# ----------------------------------------------------------------------------------------------------------- 2. with holds
@pytest.mark.parametrize("name,K,CS,holds", [
    ("keyframe 0 holds everything, keyframe 3 its code", 8, 16, {0: 7, 3: 2}),
    ("the same, B = 39", 6, 32, {0: 7, 2: 2}),
    ("every keyframe holds its code (compact rows)", 8, 16, {k: 2 for k in range(8)}),
])
def test_products_and_candidate_with_holds(capi, name, K, CS, holds):
    win, w, A, g, held, gadd, gp = general_window(capi, K, CS, [(0, K - 1)], holds=holds)
    assert held.sum() > 0 and (win.Bs < win.B) == (len(holds) == K)
    dots, gd, Agd, nd, And = check_products(capi, name, win, w, A, g, held, gadd, gp)
    for v in (gd, Agd, nd, And):
        assert not v[held].any()
    before = all_vars(win)
    for a, b in ((0.3, 0.0), (0.2, 0.6), (0.0, 1.0)):
        win.dogleg_candidate(a, b)
        d = win.delta()
        assert not d[held].any() and d[~held].all()
        assert np.all(np.abs(d - (a * gd + b * nd)) <= 4 * EPS64 * (np.abs(a * gd) + np.abs(b * nd)))
    win.accept()
    after = all_vars(win)
    B = win.B
    for k, mask in holds.items():                                      # held variables: the same bits
        (p0, c0, s0), (p1, c1, s1) = before[k], after[k]
        assert (not mask & 1) or np.array_equal(p0, p1)
        assert (not mask & 2) or np.array_equal(c0, c1)
        assert (not mask & 4) or s0 == s1
    assert not same_vars(before, after)
    win.close()


# ----------------------------------------------------------------------------------------------------------- 3. the candidate
@pytest.mark.parametrize("K,CS", [(46, 16), (27, 32)])
def test_candidate_against_the_blend_and_the_solve(capi, K, CS):
    """K * B = 1058 and 1053: both reach the second stride of the candidate kernel's entry loop"""
    B = 7 + CS
    assert K * B > 1024
    win, w, A, g, held, gadd, gp = general_window(capi, K, CS, [(0, K - 1)])
    before = all_vars(win)
    win.solve(0.0)
    solved = win.delta()
    dots = win.dogleg_products()
    gd, Agd, nd, And = win.dogleg_vectors()
    nu, nn = dots[0] / dots[3] * np.sqrt(dots[0]), np.sqrt(dots[2])
    assert nu < nn
    worst = 0.0
    for delta, region in ((0.5 * nu, 0), (0.5 * (nu + nn), 1), (2.0 * nn, 2)):
        rc, a, b, reg = capi.dogleg_point(delta, *dots[:4])
        assert (rc, reg) == (0, region)
        win.dogleg_candidate(a, b)
        d = win.delta()
        bar = 4 * EPS64 * (np.abs(a * gd) + np.abs(b * nd))
        err = np.abs(d - (a * gd + b * nd))
        worst = max(worst, float(np.max(err / bar)))
        assert np.all(err <= bar), (region, worst)
        if region < 2:
            assert abs(np.linalg.norm(d) - delta) <= 1e-12 * delta
    summary_line(f"dogleg candidate K {K} CS {CS}: delta vs a g + b n {worst:.2f} of the bar 4 eps (|a g| + |b n|)")
    # the last candidate is (0, 1): the bits of solve(0) alone, in the delta mirror and in the variables
    assert (a, b) == (0.0, 1.0)
    assert np.array_equal(d, solved) and np.array_equal(np.signbit(d), np.signbit(solved))
    win.accept()
    got = all_vars(win)
    twin, *_ = general_window(capi, K, CS, [(0, K - 1)])
    nrm = twin.solve(0.0)
    assert np.array_equal(twin.delta(), solved) and abs(nrm - np.linalg.norm(solved)) <= 1e-12 * nrm
    twin.accept()
    want = all_vars(twin)
    assert same_vars(got, want) and not same_vars(got, before)
    for (p, c, s), (q, e, t) in zip(got, want):
        assert np.array_equal(np.signbit(c), np.signbit(e))
    # ... and on the device: the next linearize reads the same variables
    win.linearize(); twin.linearize()
    assert np.array_equal(win.packed_host(), twin.packed_host())
    # a steepest-descent candidate: codes and scales one fp32 add of the fp32-rounded step, poses at the fp32 oracle's distance
    rc, a, b, reg = capi.dogleg_point(0.5 * nu, *dots[:4])
    third, *_ = general_window(capi, K, CS, [(0, K - 1)])
    assert same_vars(all_vars(third), before)
    third.solve(0.0, want_norm=False)
    assert np.array_equal(third.dogleg_products(), dots)
    third.dogleg_candidate(a, b)
    step = third.delta().reshape(K, B)
    assert abs(np.linalg.norm(step) - 0.5 * nu) <= 1e-12 * nu
    third.accept()
    for k, ((p0, c0, s0), (p1, c1, s1)) in enumerate(zip(before, all_vars(third))):
        assert np.array_equal(c1, c0 + step[k, 6:6 + CS].astype(np.float32)), k
        assert np.float32(s1) == np.float32(s0) + np.float32(step[k, 6 + CS]), k
        r64 = retract_ref(p0, step[k, :6])
        e_ref = np.abs(retract_ref_f32(p0, step[k, :6]).astype(np.float64) - r64).max()
        theta = float(np.linalg.norm(step[k, 3:6].astype(np.float32).astype(np.float64)))
        bar = 4 * e_ref + 8 * EPS32 * max(1.0, np.abs(r64[9:]).max())  # (test_device_retraction_at_chosen_steps' bars)
        bar_t = bar + (EPS32 * float(np.linalg.norm(step[k, :3])) / theta if theta > 0 else 0.0)
        dist = np.abs(p1.astype(np.float64) - r64)
        assert dist[:9].max() <= bar and dist[9:].max() <= bar_t, (k, dist.max(), e_ref)
    win.close(); twin.close(); third.close()


# ------------------------------------------------------------------------------------------------------- 4. a step replayed
def test_five_steps_replayed(capi):
    """K = 6, CS = 32, the default priors.  A twin window walks the same iterates through the primitives (linearize, solve(0),
    products, candidate, accept): what the step accepts is what accept() leaves there."""
    import torch
    K, CS = 6, 32
    B = 7 + CS
    w = small_window(K, CS, extra=[(0, K - 1)])
    win, twin = capi.Window(w), capi.Window(w)
    deg = np.zeros(K, int)
    for a, b in w.links:
        deg[a] += 1
        deg[b] += 1
    row_terms = np.repeat(2.0 * (deg + 1) * B * EPS64, B)
    cfg = capi.dogleg_config_default()
    st = capi.SageDoglegState()
    errors = []
    for it in range(5):
        cur = all_vars(win)
        assert same_vars(cur, all_vars(twin))
        win.linearize()
        lin = win.packed_host().astype(np.float64)
        delta_in = st.delta if st.delta > 0 else cfg.init_delta
        win.dogleg_step(st, cfg)
        # The step linearizes as the classic LM sequence does, with the merged kernel of the two factor types, whose fp32 sums
        # differ from sage_window_linearize's in their last bits: A and g are rebuilt from the system the step solved (the
        # classic sequence leaves it in `packed`, also behind an accept), which is linearize()'s to fp32 accuracy
        packed = win.packed_host().astype(np.float64)
        assert rel(packed[:-4], lin[:-4]) <= 1e-5
        dadd, gadd = prior_vectors(w, CS, code_w=CODE_W, codes=[c[1] for c in cur], pose0=cur[0][0], scale0=cur[0][2])
        A, g, held = ref.dense_system(capi, packed, w.links, K, CS, dadd, gadd)
        dots = np.array(st.dots)
        gd, Agd, nd, And = win.dogleg_vectors()
        # the bars of 1.
        worst = {}
        for tag, prod, v in (("Ag", Agd, gd), ("An", And, nd)):
            bar = row_terms * (np.abs(A) @ np.abs(v))
            err = np.abs(prod - A @ v)
            worst[tag] = float(np.max(err / bar))
            assert np.all(err <= bar), (it, tag, worst[tag])
        for got, (x, y) in zip(dots, ((gd, gd), (gd, nd), (nd, nd), (gd, Agd), (gd, And), (nd, And))):
            assert abs(got - float(x @ y)) <= 2.0 * K * B * EPS64 * float(np.sum(np.abs(x * y)))
        # the policy replayed on the reported errors.  ONE_STEP_PER_ITERATION evaluates again only after an error that rose:
        # every evaluation but the last is replayed as one -- and the last too when the zero step was taken, whose reported
        # candidate error is the error kept (near convergence the fp32 error pass cannot resolve the decrease any more)
        calls = []

        def reported(a, b):
            calls.append((a, b))
            return st.candidate_error if len(calls) == st.evals and st.accepted else st.error + 1.0

        want = ref.iterate(delta_in, cfg.mode, dots, st.error, reported)
        assert st.evals == want["evals"] == len(calls) and st.accepted == want["accepted"] and st.region == want["region"]
        if st.accepted:
            assert abs(st.rho - want["rho"]) <= 1e-12 * abs(want["rho"]), it
        else:
            assert st.candidate_error == st.error and st.rho < 0 and st.delta <= cfg.min_delta and st.step_norm == 0.0
        for name in ("delta", "a", "b"):
            assert abs(getattr(st, name) - want[name]) <= 1e-12 * abs(want[name]), (it, name)
        # delta: the point of the last evaluation, within the bar of 3.
        a, b = calls[-1]
        d = win.delta()
        bar = 4 * EPS64 * (np.abs(a * gd) + np.abs(b * nd))
        assert np.all(np.abs(d - (a * gd + b * nd)) <= bar)
        # the twin through the primitives, on the step's system
        twin.linearize()
        torch.cuda.synchronize()
        twin.packed_tensor().copy_(win.packed_tensor())
        torch.cuda.synchronize()
        twin.solve(0.0, want_norm=False)
        assert np.array_equal(twin.dogleg_products(), dots)
        twin.dogleg_candidate(a, b)
        assert np.array_equal(twin.delta(), d)
        if st.accepted:
            twin.accept()
        assert same_vars(all_vars(win), all_vars(twin)) and same_vars(all_vars(win), cur) == (not st.accepted)
        assert st.solves == st.iters == it + 1
        assert st.candidate_error <= st.error
        errors.append((st.error, st.candidate_error))
        summary_line(f"dogleg step {it + 1}: error {st.error:.6f} -> {st.candidate_error:.6f}, rho {st.rho:.4f}, region "
                     f"{st.region}, evals {st.evals}, radius {delta_in:.4g} -> {st.delta:.4g}, |step| {st.step_norm:.4g} "
                     f"(|u| {st.sd_norm:.3g}, |n| {st.gn_norm:.3g}); Ag {worst['Ag']:.2f}, An {worst['An']:.2f} of their bars")
    assert all(e1[0] <= e0[0] for e0, e1 in zip(errors, errors[1:]))   # the error never rises
    assert errors[-1][1] < errors[0][0]
    win.close(); twin.close()


def test_run_matches_the_steps(capi):
    """sage_window_dogleg_run is n steps: the same trace, the same variables"""
    w = small_window(4, 16)
    a, b = capi.Window(w), capi.Window(w)
    cfg = capi.dogleg_config_default()
    sa, sb = capi.SageDoglegState(), capi.SageDoglegState()
    tr = a.dogleg_run(sa, cfg, 3)
    rows = []
    for _ in range(3):
        b.dogleg_step(sb, cfg)
        rows.append([sb.error, sb.candidate_error, sb.accepted, sb.delta, sb.rho, sb.region, sb.evals])
    assert tr.shape == (3, 7) and np.array_equal(tr, np.array(rows, np.float64))
    assert same_vars(all_vars(a), all_vars(b)) and (sa.solves, sa.iters) == (3, 3)
    a.close(); b.close()


def test_a_non_positive_pivot_leaves_window_and_state_alone(capi, orc):
    """test_gpu_window_candidate.py's keyframe that lost overlap: its pose and scale rows are zero, the Gauss-Newton
    factorisation fails; the step answers SAGE_E_NOT_PSD, nothing has moved, and after the keyframe is put back it walks"""
    w, wl, _ = lost_scene(orc, 32)
    win = capi.Window(w)
    start = all_vars(win)
    gone = wl.keyframes[3]
    win.set_keyframe(3, capi.pack_pose(gone.R, gone.t), start[3][1], start[3][2])
    lost = all_vars(win)
    st, cfg = capi.SageDoglegState(), capi.dogleg_config_default()
    st.delta = 0.5
    before = bytes(st)
    for _ in range(2):
        with pytest.raises(capi.SageError) as err:
            win.dogleg_step(st, cfg)
        assert err.value.code == NOT_PSD and bytes(st) == before and same_vars(all_vars(win), lost)
    win.set_keyframe(3, *start[3])
    win.dogleg_step(st, cfg)
    assert (st.iters, st.solves, st.accepted) == (1, 1, 1) and st.candidate_error < st.error
    win.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("name", ["sharded", "reduced", "duplicate link"])
def test_unsupported_windows_refuse_and_keep_working(capi, name):
    w = small_window(4, 16)
    if name == "duplicate link":
        w = dataclasses.replace(w, links=list(w.links) + [w.links[1]])
    win = capi.Window(w, rank=0, world=2 if name == "sharded" else 1)
    rec = None
    if name != "duplicate link":
        rec = _Recorder()
        win.set_allreduce(rec)
        rec.step()
    start = all_vars(win)
    st, cfg = capi.SageDoglegState(), capi.dogleg_config_default()
    for call in (lambda: win.dogleg_step(st, cfg), lambda: win.dogleg_run(st, cfg, 2), win.dogleg_products,
                 lambda: win.dogleg_candidate(0.0, 1.0), win.dogleg_vectors):
        with pytest.raises(capi.SageError) as err:
            call()
        assert err.value.code == UNSUPPORTED
    assert (st.iters, st.solves, st.delta) == (0, 0, 0.0) and same_vars(all_vars(win), start)
    lst, lcfg = capi.SageLmState(), capi.lm_config_default()
    if rec is not None:
        rec.step()
    win.lm_step(lst, lcfg)
    assert lst.iters == 1 and np.isfinite(lst.error)
    if name != "sharded":                                              # (rank 0 of two walks with its share of the links only)
        assert lst.accepted == 1 and lst.candidate_error < lst.error
    win.close()
