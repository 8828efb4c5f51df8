"""From a damped system to a candidate on the GPU, and what happens when there is no candidate.

The suite follows a window's solve up to `delta` (tests/test_gpu_parity.py, tests/test_gpu_window_solver_rows.py).  These tests
look at what comes after it -- the retract kernel's candidate poses, codes and scales -- and at the solve that fails.
`Window.packed_tensor()` is a writable view of the device's packed buffer: 1. and 2. hand the scatter, the host factorisation
and the retract a well-conditioned system of their own choosing, so the comparison runs near machine precision and the
retraction sees the steps the test picks (rotation angles from 0 past 2 pi, exact zeros).

1. the device retraction at chosen steps: delta, its norm, codes and scales bit for bit, poses against the fp64 reference
   (tests/helpers.py retract_ref) by a bar measured in the fp32 oracle's own distance from it; the host mirror and the device
   copy of the accepted variables are the same bits.
2. an injected general system (asymmetric diagonal storage, fill blocks, padded blocks, priors with a gradient) against a dense
   numpy solve at 64 eps cond(A).
3. a keyframe that lost overlap: its pose and scale rows are exactly zero, every damped solve fails with SAGE_E_NOT_PSD, in the
   direct calls and in each LM sequence; nothing moves, the errors stay those of the oracle, the collectives are the documented
   ones, and after the keyframe is put back the window walks on bit for bit like one that never failed.
4. a new run length (sage_window_set_runs) drops the system assembled under the previous one.

Measured on an MI355X (summary_line prints the figures on every run):
1. largest distance of the engine's / the fp32 oracle's pose from fp64, and the worst ratio on one keyframe, per angle:
     angle         K = 27, CS = 32               K = 46, CS = 16
     0             3.0e-8 / 3.0e-8  (1.00)       1.5e-8 / 1.5e-8  (1.00)
     1e-20         7.5e-9 / 7.5e-9  (1.00)       1.5e-8 / 1.5e-8  (1.00)
     1e-7          1.8e-8 / 1.8e-8  (1.00)       2.5e-8 / 2.5e-8  (1.00)
     1e-3          5.2e-6 / 5.2e-6  (1.00)       6.4e-6 / 6.4e-6  (1.00)
     1e-2          2.6e-7 / 2.6e-7  (1.00)       2.2e-7 / 2.2e-7  (1.01)
     0.3           7.1e-8 / 6.0e-8  (1.80)       6.2e-8 / 8.7e-8  (1.13)
     3             1.1e-7 / 1.1e-7  (1.12)       3.6e-7 / 2.9e-7  (3.17)
     pi - 1e-3     1.1e-7 / 7.3e-8  (1.52)       3.1e-7 / 2.6e-7  (2.03)
     pi            1.6e-7 / 1.6e-7  (1.00)       2.2e-7 / 2.2e-7  (1.37)
     4             1.1e-7 / 1.1e-7  (1.00)       2.2e-7 / 1.7e-7  (1.81)
     2 pi + 0.1    2.9e-7 / 2.9e-7  (1.00)       2.4e-7 / 2.4e-7  (1.00)
   At 1e-7 and below the engine is at the oracle's distance: the device's cosf is 1 there and the reference formula keeps
   the translation.  Delta, its norm, codes, scales and the mirror / device copy met their bars exactly as stated.
2. device solve vs numpy: K = 18, CS = 16: 6.4e-16 (damp 0.5, cond(A) 13.4, bar 1.9e-13), 7.6e-16 (1e-3, cond 15.0, bar
   2.1e-13); K = 6, CS = 32: 6.9e-16 (0.5, cond 13.7), 6.6e-16 (1e-3, cond 16.0).  The reference takes the code prior weight
   as the config's float holds it, float32(1e-3): with the double 1e-3 it is 3.1e-11 away.
3. error with keyframe 3 gone 1089.5645 (CS = 32; 1088.9809 at CS = 16, 1091.2434 with the duplicate link), the oracle's to
   all printed digits; after the keyframe is put back 13.089660 -> 4.825949, as on a fresh window, in every bit.
4. the window is the first one tried, K = 4 at 64 x 80, FS = 16: the rule's run length is 1, runs of 4 move the packed buffer
   by up to 3.3e-3 (absolute); the step after the change 110.269087 -> 15.670434 on both windows."""
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import synth
from tests.conftest import summary_line
from tests.helpers import oracle_geo, oracle_photo, pose_local, prior_vectors, rel, retract_ref, retract_ref_f32
from tests.test_gpu_sharded_lm import _Recorder

pytestmark = pytest.mark.gpu

EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
CODE_W = float(np.float32(1e-3))                                 # the code prior weight as SageWindowConfig's float holds it
NOT_PSD = -3                                                     # SAGE_E_NOT_PSD


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


def small_window(K, CS, extra=()):
    """the shape of test_long_window_lm: 24 x 32 images, two levels, 300 samples, links to the three keyframes before"""
    w = synth.make_window(K=K, H=24, W=32, FS=16, CS=CS, L=2, n_samples=300, seed=41, back_links=3)
    for lk in extra:
        if lk not in w.links:
            w.links.append(lk)
    return w


def all_vars(win):
    return [win.get_keyframe(k) for k in range(win.K)]


def same_vars(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))


def inject(win, diag, lnk, g):
    """overwrite the device's packed system [K diag blocks | link blocks | gradient | 4 totals] behind a linearize (the
    window then counts as linearized); the totals are zero"""
    import torch
    win.linearize()
    torch.cuda.synchronize()
    packed = np.concatenate([np.asarray(diag, np.float64).ravel(), np.asarray(lnk, np.float64).ravel(),
                             np.asarray(g, np.float64).ravel(), np.zeros(4)])
    assert packed.size == win.packed_count
    win.packed_tensor().copy_(torch.from_numpy(packed).cuda())
    torch.cuda.synchronize()
    return packed


# ------------------------------------------------------------------------------------------------ 1. the device retraction
ANGLES = [0.0, 1e-20, 1e-7, 1e-3, 1e-2, 0.3, 3.0, np.pi - 1e-3, np.pi, 4.0, 2 * np.pi + 0.1]
ZERO_POSE_STEP = 11                                              # this keyframe's pose step is all zero (its angle is 0 anyway)


def chosen_steps(K, CS, seed):
    """[K, B] steps: keyframe k turns by ANGLES[k mod 11] about a seeded axis and moves by 0.3; code and scale steps
    N(0, 1e-2) with three exact zeros per keyframe"""
    rng = np.random.default_rng(seed)
    d = np.zeros((K, 7 + CS))
    for k in range(K):
        axis, v = rng.standard_normal(3), rng.standard_normal(3)
        d[k, :3] = 0.3 * v / np.linalg.norm(v)
        d[k, 3:6] = ANGLES[k % len(ANGLES)] * axis / np.linalg.norm(axis)
        d[k, 6:] = rng.normal(0.0, 1e-2, CS + 1)
        d[k, 6 + rng.choice(CS + 1, 3, replace=False)] = 0.0
    d[ZERO_POSE_STEP, :6] = 0.0
    return d


@pytest.mark.parametrize("K,CS", [(27, 32), (46, 16)])
def test_device_retraction_at_chosen_steps(capi, orc, K, CS):
    """K * B = 1053 (B = 39) and 1058 (B = 23, padded to 24): both reach the second stride of the retract kernel's entry loop.
    Identity diagonal blocks, no priors, damping 1: A = 2 I, and the gradient 2 * delta_want makes delta_want the solution."""
    B = 7 + CS
    assert K * B > 1024
    w = small_window(K, CS)
    win = capi.Window(w, code_prior_weight=0.0, scale_prior_weight=0.0, pose_prior_weight=0.0)
    want = chosen_steps(K, CS, seed=K)
    inject(win, np.tile(np.eye(B), (K, 1, 1)), np.zeros((len(w.links), B, B)), 2.0 * want)
    before = all_vars(win)
    nrm = win.solve(1.0)
    delta = win.delta()
    # delta and its norm
    assert np.all(np.abs(delta - want.ravel()) <= 4 * EPS64 * np.abs(want.ravel()))
    assert np.array_equal(delta == 0.0, want.ravel() == 0.0) and np.count_nonzero(delta == 0.0) >= 3 * K + 6
    assert abs(nrm - np.linalg.norm(delta)) <= 1e-12 * np.linalg.norm(delta)
    win.accept()
    after = all_vars(win)
    delta = delta.reshape(K, B)
    worst = {}                                                   # angle -> [engine distance, oracle distance, their ratio]
    for k in range(K):
        (p0, c0, s0), (p1, c1, s1) = before[k], after[k]
        # codes and scales: one fp32 add of the fp32-rounded step
        assert np.array_equal(c1, c0 + delta[k, 6:6 + CS].astype(np.float32)), k
        assert np.float32(s1) == np.float32(s0) + np.float32(delta[k, 6 + CS]), k
        # the pose against the fp64 reference, in units of the fp32 oracle's own distance from it
        d6 = delta[k, :6]
        ref = retract_ref(p0, d6)
        e_ref = np.abs(retract_ref_f32(p0, d6).astype(np.float64) - ref).max()
        dist = np.abs(p1.astype(np.float64) - ref)
        theta = float(np.linalg.norm(d6[3:].astype(np.float32).astype(np.float64)))
        bar = 4 * e_ref + 8 * EPS32 * max(1.0, np.abs(ref[9:]).max())
        bar_t = bar + (EPS32 * float(np.linalg.norm(d6[:3])) / theta if theta > 0 else 0.0)
        a = ANGLES[k % len(ANGLES)]
        rec = worst.setdefault(a, [0.0, 0.0, 0.0])
        rec[0], rec[1] = max(rec[0], dist.max()), max(rec[1], e_ref)
        rec[2] = max(rec[2], dist.max() / e_ref if e_ref > 0 else (0.0 if dist.max() == 0 else np.inf))
        print(f"K {K} keyframe {k} angle {a:.3g}: engine {dist[:9].max():.2e} (R) {dist[9:].max():.2e} (t), fp32 oracle "
              f"{e_ref:.2e}, bars {bar:.2e} / {bar_t:.2e}")
        assert dist[:9].max() <= bar and dist[9:].max() <= bar_t, (k, a, dist.max(), e_ref)
    summary_line(f"device retraction K {K} CS {CS}, engine / fp32-oracle distance from fp64 per angle (worst ratio): " + ", ".join(
        f"{a:.7g}: {v[0]:.1e} / {v[1]:.1e} ({v[2]:.2f})" for a, v in worst.items()))
    # the host mirror (get_keyframe) and the device copy (what the next linearize reads) hold the same variables
    win.linearize()
    kfs = [dataclasses.replace(kf, R=p[:9].reshape(3, 3).copy(), t=p[9:].copy(), code=c.copy(), scale=s)
           for kf, (p, c, s) in zip(w.keyframes, after)]
    twin = capi.Window(dataclasses.replace(w, keyframes=kfs), code_prior_weight=0.0, scale_prior_weight=0.0,
                       pose_prior_weight=0.0)
    twin.linearize()
    assert np.array_equal(twin.packed_host(), win.packed_host())
    win.close(); twin.close()


# ------------------------------------------------------------------------------------------- 2. an injected general system
@pytest.mark.parametrize("K,CS", [(18, 16), (6, 32)])
def test_injected_system_against_a_dense_solve(capi, K, CS):
    """K = 18: a split plan with structural fill blocks, B = 23 padded to 24; K = 6: B = 39; both with the loop link (0, K - 1).
    Code prior 1e-3, pose and scale prior 10 on a keyframe 0 that has moved, so that each prior has a gradient."""
    B = 7 + CS
    w = small_window(K, CS, extra=[(0, K - 1)])
    win = capi.Window(w, code_prior_weight=CODE_W, scale_prior_weight=10.0, pose_prior_weight=10.0)
    p0, c0, s0 = win.get_keyframe(0)
    win.set_keyframe(0, retract_ref_f32(p0, [0.01, -0.02, 0.015, 0.02, 0.01, -0.03]), c0, float(np.float32(1.05 * s0)))
    cur = all_vars(win)
    rng = np.random.default_rng(100 + K)
    diag = np.stack([np.diag(1.0 + rng.uniform(0, 1, B)) + 0.02 * rng.standard_normal((B, B)) for _ in range(K)])
    assert not np.array_equal(diag[0], diag[0].T)                # not symmetric in storage: the builders symmetrise
    packed = inject(win, diag, 0.02 * rng.standard_normal((len(w.links), B, B)), rng.standard_normal(K * B))
    H, g, _ = capi.unpack_dense(packed, K, w.links, CS)          # diagonal blocks as 0.5 (D + D^T)
    dadd, gadd = prior_vectors(w, CS, code_w=CODE_W, codes=[c[1] for c in cur], pose0=cur[0][0], scale0=cur[0][2],
                               pose_w=10.0, scale_w=10.0)
    assert np.abs(gadd[:6]).min() > 0 and gadd[6 + CS] != 0
    HP = H + np.diag(dadd)
    for damp in (0.5, 1e-3):
        A = HP + damp * np.diag(np.diag(HP))
        cond = float(np.linalg.cond(A))
        assert cond < 100
        ref = np.linalg.solve(A, g + gadd)
        win.solve(damp)
        d = rel(win.delta(), ref)
        summary_line(f"injected system K {K} CS {CS} damp {damp}: device solve vs numpy {d:.2e}, cond(A) {cond:.1f}, bar "
                     f"{64 * EPS64 * cond:.2e}")
        assert d <= 64 * EPS64 * cond
    win.close()


# --------------------------------------------------------------------------------------- 3. a keyframe that lost overlap
_LOST = {}


def lost_scene(orc, CS):
    """the window with its good poses, the same with keyframe 3 moved 50 to the side (t + R [50, 0, 0]: no pixel of it
    projects into a neighbour or back), and the oracle's result of every edge of the moved window -- computed once per CS"""
    if CS not in _LOST:
        w = synth.make_window(K=4, H=32, W=40, FS=16, CS=CS, L=3, seed=7, back_links=2)
        kf = w.keyframes[3]
        gone = dataclasses.replace(kf, t=(kf.t + kf.R @ np.array([50, 0, 0], np.float32)).astype(np.float32))
        wl = dataclasses.replace(w, keyframes=w.keyframes[:3] + [gone])
        res = {}
        for l, (a, b) in enumerate(wl.links):
            for d, (k0, k1) in enumerate(((a, b), (b, a))):
                res[(0, l, d)] = oracle_photo(orc, wl, k0, k1)
                res[(1, l, d)] = oracle_geo(orc, wl, k0, k1)
        _LOST[CS] = (w, wl, res)
    return _LOST[CS]


def prior_error(win, w, code_w=CODE_W, scale_w=1e4, pose_w=1e4):
    """window_prior_error at the window's current variables, written out: w ||c||^2 / CS per keyframe, on keyframe 0
    w (ln s_init - ln s)^2 and w |pose_local(pose, pose_init)|^2"""
    e = 0.0
    for k in range(win.K):
        c = win.get_keyframe(k)[1].astype(np.float64)
        e += code_w * float(c @ c) / w.CS
    p0, _, s0 = win.get_keyframe(0)
    kf0 = w.keyframes[0]
    e += scale_w * (np.log(float(np.float32(kf0.scale))) - np.log(float(s0))) ** 2
    init = np.concatenate([np.asarray(kf0.R, np.float32).ravel(), np.asarray(kf0.t, np.float32).ravel()])
    return e + pose_w * float(np.sum(pose_local(p0, init) ** 2))


# name -> (CS, linearize_at_candidate, behind a recording hook, a link added twice)
LOST_CASES = {"classic": (32, -1, False, False), "classic CS 16": (16, -1, False, False), "at candidate": (32, 1, False, False),
              "classic behind a hook": (32, -1, True, False), "automatic behind a hook": (32, 0, True, False),
              "classic, duplicate link": (32, -1, False, True)}


@pytest.mark.parametrize("name", list(LOST_CASES))
def test_lost_keyframe_fails_every_solve_and_recovers(capi, orc, name):
    CS, variant, hooked, duplicate = LOST_CASES[name]
    w, wl, res = lost_scene(orc, CS)
    links = list(w.links)
    if duplicate:                                                # no device solver: the window solves on the host
        links.append(links[1])
        res = dict(res)
        for t in (0, 1):
            for d in (0, 1):
                res[(t, len(links) - 1, d)] = res[(t, 1, d)]
    K, B = 4, 7 + CS
    at_candidate = variant > 0 or (variant == 0 and hooked)

    def build():
        win = capi.Window(dataclasses.replace(w, links=list(links)))
        rec = _Recorder() if hooked else None
        if rec is not None:
            win.set_allreduce(rec)
            rec.step()
        return win, rec

    def step(win, rec, st):
        cfg = capi.lm_config_default()
        cfg.linearize_at_candidate = variant
        if rec is not None:
            rec.step()
        win.lm_step(st, cfg)
        return cfg

    win, rec = build()
    start = all_vars(win)
    gone = wl.keyframes[3]
    win.set_keyframe(3, capi.pack_pose(gone.R, gone.t), start[3][1], start[3][2])
    win.linearize()
    # the system and the totals: the oracle's
    n_lost = 0
    for l, (a, b) in enumerate(links):
        for d in (0, 1):
            if 3 not in (a, b):
                continue
            for t, fallback in ((0, 10.0 * float(w.photo_weights.sum())), (1, 10.0 * w.geo_weight)):
                o, h = res[(t, l, d)], win.get_edge(t, 2 * l + d)
                assert o["num_inliers"] == 0 and h["num_inliers"] == 0
                assert o["error"] == pytest.approx(fallback, rel=1e-6) and h["error"] == pytest.approx(o["error"], rel=2e-5)
                assert not h["AtA"].any() and not h["Atb"].any()
                n_lost += 1
    assert n_lost == 8
    packed = win.packed_host().astype(np.float64)
    ref = capi.assemble_packed(K, links, CS, res)
    assert np.array_equal(packed[-2:], ref[-2:]) and packed[-4:-2] == pytest.approx(ref[-4:-2], rel=2e-5)
    D3 = packed[3 * B * B:4 * B * B].reshape(B, B)
    assert not D3[:6].any() and not D3[:, :6].any() and not D3[B - 1].any() and not D3[:, B - 1].any()
    e_ref = ref[-4] + ref[-3] + prior_error(win, w)
    lost = all_vars(win)
    e_lin = win.total_error(True)
    assert e_lin == pytest.approx(e_ref, rel=2e-5)
    # the direct solve
    for want_norm in (True, False):
        with pytest.raises(capi.SageError) as err:
            win.solve(1e-3, want_norm=want_norm)
        assert err.value.code == NOT_PSD
        assert win.total_error(True) == e_lin and same_vars(all_vars(win), lost)
    # two LM steps: every evaluation is a rejected one
    st = capi.SageLmState()
    cfg = step(win, rec, st)
    first_error = st.error
    assert (st.accepted, st.iters) == (0, 1) and st.candidate_error == np.inf and st.damp == float(cfg.max_damp)
    assert st.error == pytest.approx(e_ref, rel=2e-5) and same_vars(all_vars(win), lost)
    step(win, rec, st)
    assert (st.accepted, st.iters) == (0, 2) and st.candidate_error == np.inf and st.damp == float(cfg.max_damp)
    assert st.error == first_error and same_vars(all_vars(win), lost)
    if rec is not None:                                          # the collectives (include/sage_ba.h: SageAllReduceFn)
        npk = win.packed_count
        assert npk != 4 and rec.steps == ([[], [npk], []] if at_candidate else [[], [npk], [npk]]), rec.steps
    # recovery: the keyframe is put back; the window walks on like one that never failed
    win.set_keyframe(3, *start[3])
    assert same_vars(all_vars(win), start)
    st = capi.SageLmState()
    step(win, rec, st)
    fresh, frec = build()
    fst = capi.SageLmState()
    step(fresh, frec, fst)
    assert st.accepted == 1 and fst.accepted == 1
    summary_line(f"lost keyframe, {name}: error with keyframe 3 gone {first_error:.4f} (oracle {e_ref:.4f}); after it is put "
                 f"back {st.error:.6f} -> {st.candidate_error:.6f}, a fresh window {fst.error:.6f} -> {fst.candidate_error:.6f}")
    assert (st.error, st.candidate_error, st.damp, st.iters) == (fst.error, fst.candidate_error, fst.damp, fst.iters)
    assert np.array_equal(win.delta(), fresh.delta()) and np.linalg.norm(win.delta()) > 0
    assert same_vars(all_vars(win), all_vars(fresh)) and not same_vars(all_vars(win), start)
    if rec is not None:
        assert rec.steps[3] == frec.steps[1] and len(rec.steps) == 4 and len(frec.steps) == 2
    win.close(); fresh.close()


# ------------------------------------------------------------------------------------------ 4. a plan change and the system
def test_a_new_run_length_drops_the_system_assembled_under_the_old_one(capi):
    """K = 4 at 64 x 80, FS = 16 -- the smallest window tried: the rule's run length there is 1 sub-tile per workgroup, and
    runs of 4 sum the photometric partial results in another fp32 order (the packed buffers differ, asserted first).  A
    window linearized under the rule's run length and then given the other one must not solve the old system: the
    linearize-at-candidate sequence, which reuses a system that is booked as current, walks like a window that got its run
    length before it ever linearized."""
    w = synth.make_window(K=4, H=64, W=80, FS=16, CS=32, L=4, seed=71)
    probe = capi.Window(w)
    t1 = probe.tune_runs()["tpb_rule"]
    probe.close()
    t2 = 4 if t1 != 4 else 2
    packed = {}
    for t in (t1, t2):
        win = capi.Window(w)
        win.set_runs(t)
        win.linearize()
        packed[t] = win.packed_host()
        win.close()
    assert not np.array_equal(packed[t1], packed[t2])            # the precondition: the run length shows in the bits
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    cfg.linearize_at_candidate = 1
    a, b = capi.Window(w), capi.Window(w)
    a.set_runs(t2)
    b.linearize()
    assert np.array_equal(b.packed_host(), packed[t1])
    b.set_runs(t2)
    sa, sb = capi.SageLmState(), capi.SageLmState()
    a.lm_step(sa, cfg); b.lm_step(sb, cfg)
    summary_line(f"run lengths {t1} (rule) -> {t2} on K 4, 64 x 80: packed buffers differ by "
                 f"{np.abs(packed[t1] - packed[t2]).max():.2e}; step after the change {sb.error:.6f} -> {sb.candidate_error:.6f}, "
                 f"run length set first {sa.error:.6f} -> {sa.candidate_error:.6f}")
    assert sa.accepted == 1
    assert (sa.error, sa.candidate_error, sa.accepted, sa.damp) == (sb.error, sb.candidate_error, sb.accepted, sb.damp)
    assert np.array_equal(a.delta(), b.delta()) and same_vars(all_vars(a), all_vars(b))
    b.linearize()
    b.set_runs(t1)
    with pytest.raises(capi.SageError) as err:                   # nothing to solve until a linearize has followed
        b.solve(1e-3)
    assert err.value.code == -4                                  # SAGE_E_STATE
    a.close(); b.close()
