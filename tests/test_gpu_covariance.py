"""Marginal covariances on the GPU (include/sage_ba.h "marginal covariances"): sage_window_covariance / _get_covariance against
numpy.linalg.inv of the dense system the solve factorised (tests/covariance_ref.py over marginal_ref.dense_system), and the
depth variance / sigma maps (depth_sigma_kernel) against j'Sj in fp64.

Windows: synth.make_window(K, H=24, W=32, FS=16, L=2, n_samples=300, back_links=3), as tests/test_gpu_marginal_prior.py.

Bars.
* Sigma: ||Sigma_hat - Sigma||_F <= 64 n 2^-53 cond_2(M) ||Sigma||_2 for every diagonal and every link block, n the rows of
  the system that was factorised (K B; the free rows of a window that holds some), cond_2 computed in the test.
* var: |var - var64| <= gamma_N |j|'|S~||j|, N = 3 (CS + 1) + 4 fp32 roundings (the dot product that forms j, the
  matrix-vector product, the outer dot product), var64 formed in fp64 from the fp32-rounded inputs; sigma within 1 ulp of
  sqrt(max(var, 0)) of the variance-mode output.
Every run prints the measured distances through conftest.summary_line."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import covariance_ref as R
from tests import marginal_ref as M
from tests.conftest import summary_line

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOT_PSD, STATE = -1, -2, -3, -4
CODE_W, SCALE_W, POSE_W = 1.0e-3, 1.0e4, 1.0e4           # capi.Window's defaults
HOLD_POSE, HOLD_CODE, HOLD_SCALE = 1, 2, 4


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


def scene(K, CS, extra=()):
    w = synth.make_window(K=K, H=24, W=32, FS=16, CS=CS, L=2, n_samples=300, seed=41, back_links=3)
    return dataclasses.replace(w, links=list(w.links) + [lk for lk in extra if lk not in w.links])


def variables(win):
    v = [win.get_keyframe(k) for k in range(win.K)]
    return (np.array([p for p, _c, _s in v]), np.array([c for _p, c, _s in v]), np.array([s for _p, _c, s in v], np.float32))


def reference(w, win, damp, hold=None, at=None):
    """Sigma [K B, K B] of the system the window's solve factorises at damping ``damp``: the inverse over the free rows,
    zeros on the held ones; with cond_2 and ||Sigma||_2 of that free system.  ``at``: the variables of the linearization
    (default: the current ones)"""
    pose, code, scl = at if at is not None else variables(win)
    kf0 = w.keyframes[0]
    dadd, gadd, _err = M.prior_rows(win.K, w.CS, pose, code, scl, CODE_W, SCALE_W, POSE_W,
                                    pose_init0=np.concatenate([kf0.R.ravel(), kf0.t]).astype(np.float32),
                                    scale_init0=np.float32(kf0.scale), hold=hold)
    H, _g = M.dense_system(win.packed_host(), win.K, win.links, w.CS, dadd, gadd, hold)
    free = np.ones(win.K * win.B, bool)
    for k, mask in (hold or {}).items():
        free[k * win.B:(k + 1) * win.B] = ~M.held_rows(mask, w.CS)
    idx = np.nonzero(free)[0]
    Sf, cond, norm2 = R.covariance(R.damped(H[np.ix_(idx, idx)], damp))
    Sigma = np.zeros_like(H)
    Sigma[np.ix_(idx, idx)] = Sf
    return Sigma, cond, norm2, idx.size, free


def compare(win, Sigma, cond, norm2, n, what):
    """every diagonal block and every link block (both ways round) under the bar -> worst distance / bar"""
    B = win.B
    bar = R.bar(n, cond, norm2)
    worst = 0.0
    for k in range(win.K):
        got = win.get_covariance(k, k)
        assert np.array_equal(got, got.T)
        worst = max(worst, float(np.linalg.norm(got - R.block(Sigma, B, k, k))))
    for a, b in win.links:
        got = win.get_covariance(a, b)
        assert np.array_equal(win.get_covariance(b, a), got.T)
        worst = max(worst, float(np.linalg.norm(got - R.block(Sigma, B, a, b))))
    summary_line(f"window covariance, {what}: cond {cond:.3g}, ||Sigma||_2 {norm2:.3g}, worst block {worst:.3g} = {worst / bar:.2g} "
                 f"of the bar {bar:.3g}")
    assert worst <= bar
    return worst / bar


# ------------------------------------------------------------------------------------------- (a), (b) the basic window
@pytest.mark.parametrize("CS", [16, 32])
def test_basic_window_and_damping(capi, CS):
    K = 6
    w = scene(K, CS, extra=[(0, 5)])
    win = capi.Window(w)
    win.linearize()
    for damp in (0.0, 1e-3):
        win.solve(damp)
        assert win.covariance() == damp
        compare(win, *reference(w, win, damp)[:4], what=f"K {K} CS {CS} damp {damp:g}")
    first = [win.get_covariance(k, k).tobytes() for k in range(K)]
    assert win.covariance() == 1e-3 and first == [win.get_covariance(k, k).tobytes() for k in range(K)]   # the same bits again
    assert win.get_covariance(0, 4, check=False)[0] == INVALID                  # no link block
    assert win.get_covariance(0, K, check=False)[0] == INVALID
    # a later linearize or accept does not invalidate Sigma: it belongs to the linearization it was solved at
    win.accept(); win.linearize()
    assert first == [win.get_covariance(k, k).tobytes() for k in range(K)]
    win.close()


@pytest.mark.parametrize("CS", [16, 32])
def test_after_an_accepted_lm_step(capi, CS):
    K = 6
    w = scene(K, CS, extra=[(0, 5)])
    win = capi.Window(w)
    at = variables(win)
    cfg = capi.lm_config_default(); cfg.max_inner_evals = 1; cfg.linearize_at_candidate = 0
    st = capi.SageLmState(); st.damp = 1e-3
    win.lm_step(st, cfg)
    assert st.accepted == 1
    assert win.covariance() == 1e-3                                            # the damping that step solved with
    compare(win, *reference(w, win, 1e-3, at=at)[:4], what=f"K {K} CS {CS} after an accepted LM step")
    win.close()


# ---------------------------------------------------------------------------------------------------------- (c) holds
def test_a_held_keyframe_has_no_variance(capi):
    K, CS = 6, 16
    w = scene(K, CS, extra=[(0, 5)])
    hold = {0: HOLD_POSE | HOLD_CODE | HOLD_SCALE}
    win = capi.Window(w, holds=hold)
    win.linearize(); win.solve(0.0); win.covariance()
    assert not win.get_covariance(0, 0).any()
    for b in (1, 2, 3, 5):
        assert not win.get_covariance(0, b).any() and not win.get_covariance(b, 0).any()
    Sigma, cond, norm2, n, _free = reference(w, win, 0.0, hold=hold)
    assert n == (K - 1) * win.B
    compare(win, Sigma, cond, norm2, n, what="keyframe 0 held")
    win.close()


def test_every_code_held_solves_seven_rows(capi):
    K, CS = 6, 32
    w = scene(K, CS, extra=[(0, 5)])
    hold = {k: HOLD_CODE for k in range(K)}
    win = capi.Window(w, holds=hold)
    assert win.Bs == 7
    win.linearize(); win.solve(0.0); win.covariance()
    Sigma, cond, norm2, n, free = reference(w, win, 0.0, hold=hold)
    assert n == 7 * K
    code = ~free[:win.B]
    for a, b in [(k, k) for k in range(K)] + win.links:
        got = win.get_covariance(a, b)
        assert not got[code, :].any() and not got[:, code].any()             # exactly zero
    compare(win, Sigma, cond, norm2, n, what="every code held (solver block 7)")
    win.close()


# ---------------------------------------------------------------------------------------------------------- (d) terms
def test_prior_term_and_its_structure_only_link(capi):
    from tests.test_marginal_host import random_spd
    K, CS = 6, 16
    w = scene(K, CS)
    kf_map = [0, 4]                                                            # no dense link between them
    assert (0, 4) not in w.links
    base = capi.Window(w)
    pose, code, scl = variables(base)
    base.close()
    rng = np.random.default_rng(5)
    n = len(kf_map) * (7 + CS)
    Lam = 50.0 * random_spd(rng, n, 1e3)
    P = capi.MarginalPrior(keyframes=kf_map, Lambda=0.5 * (Lam + Lam.T), eta=rng.normal(size=n), c=1.0, pose12=pose[kf_map],
                           code=code[kf_map], scale=scl[kf_map])
    win = capi.Window(w, prior_terms=[(P, kf_map)])
    P.close()
    assert win.links[-1] == (0, 4) and len(win.links) == len(w.links) + 1
    win.linearize(); win.solve(0.0); win.covariance()
    Sigma, cond, norm2, n_rows, _free = reference(w, win, 0.0)
    compare(win, Sigma, cond, norm2, n_rows, what="a marginal prior over (0, 4), structure-only link")
    assert np.linalg.norm(win.get_covariance(0, 4)) > 0
    win.close()


def test_keypoint_term(capi):
    K, CS = 6, 16
    w = scene(K, CS, extra=[(0, 5)])
    t = synth.make_reprojection_matches(w, *w.links[1], 64, 11)
    t.update(edge=2, weight=5.0, loss_param=0.1 * w.W * w.W)
    win = capi.Window(w, keypoint_terms=[t])
    plain = capi.Window(w)
    for x in (win, plain):
        x.linearize(); x.solve(0.0); x.covariance()
    assert not np.array_equal(win.get_covariance(1, 1), plain.get_covariance(1, 1))   # the term reached the factor
    compare(win, *reference(w, win, 0.0)[:4], what="one reprojection term")
    win.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------- (e) state
def test_state_rules(capi):
    K, CS = 4, 16
    w = scene(K, CS)
    win = capi.Window(w)
    assert win.covariance(check=False)[0] == STATE                             # before any solve
    win.linearize()
    assert win.covariance(check=False)[0] == STATE
    assert win.get_covariance(0, 0, check=False)[0] == STATE
    assert win.depth_sigma([0], check=False)[0] == STATE
    rc = capi.lib().sage_window_solve(win.h, C.c_double(-2.0), None)           # (H - 2 diag(H)) is not positive definite
    assert rc == NOT_PSD
    assert win.covariance(check=False)[0] == STATE                             # after a solve that failed
    win.solve(1e-3)
    assert win.get_covariance(0, 0, check=False)[0] == STATE                   # before sage_window_covariance
    assert win.covariance() == 1e-3
    assert win.get_covariance(0, 0, check=False)[0] == 0
    assert win.get_covariance(0, 3, check=False)[0] == 0 and win.get_covariance(3, 0, check=False)[0] == 0
    win.solve(1e-2)
    assert win.get_covariance(0, 0, check=False)[0] == STATE                   # a later solve invalidates Sigma
    assert win.depth_sigma([0], check=False)[0] == STATE
    assert win.covariance() == 1e-2
    win.set_runs(1)                                                            # drops the system
    assert win.covariance(check=False)[0] == STATE
    assert capi.window_depth_sigma_raw(win.h, None, 1, 0, None) == INVALID
    assert win.depth_sigma([0], mode=2, check=False)[0] == INVALID
    assert win.depth_sigma([K], check=False)[0] == INVALID
    win.close()
    w5 = scene(5, CS)
    win = capi.Window(w5)
    win.linearize(); win.solve(0.0); win.covariance()
    assert win.get_covariance(0, 4, check=False)[0] == INVALID                 # an unlinked pair
    win.close()


# ------------------------------------------------------------------------------------------ (f) sage_depth_sigma_batch
def cov_of(kind, CS, rng):
    n = CS + 1
    if kind == "well":
        A = rng.normal(size=(n, 2 * n))
        return 1e-3 * (A @ A.T / (2 * n) + np.eye(n))
    if kind == "correlated":                                                   # rho = 0.999: the quadratic form cancels
        sd = 10.0 ** rng.uniform(-2.0, -1.0, n)
        return np.outer(sd, sd) * (0.001 * np.eye(n) + 0.999)
    u = rng.normal(size=n) * 0.05                                              # rank one
    return np.outer(u, u)


def sigma_item(kind, CS, HW, rng):
    import torch
    basis = rng.normal(size=(HW, CS)).astype(np.float32)
    code = rng.normal(0.0, 0.5, CS).astype(np.float32)
    scale = float(np.float32(rng.uniform(0.5, 2.0)))
    bias = rng.uniform(0.5, 2.0, HW).astype(np.float32)
    S = cov_of(kind, CS, rng)
    if kind == "rank1":
        # half of the pixels: j orthogonal to u up to the rounding of the bias -> var ~ 0 of either sign: the clamp
        w_, v = np.linalg.eigh(S)
        u = v[:, -1]
        half = np.arange(HW) % 2 == 0
        b64 = basis.astype(np.float64)
        bias[half] = (-(b64 @ code.astype(np.float64)) - scale * (b64 @ u[:CS]) / u[CS]).astype(np.float32)[half]
    return (torch.from_numpy(bias).cuda(), torch.from_numpy(basis).cuda(), code, scale, S), (bias, basis, code, scale, S)


@pytest.mark.parametrize("kind", ["well", "correlated", "rank1"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (1, 257), (24, 32)])
@pytest.mark.parametrize("CS", [16, 32])
def test_depth_sigma_batch(capi, ws, CS, H, W, n, kind):
    import torch
    HW = H * W
    rng = np.random.default_rng(1000 * CS + 10 * HW + n)
    made = [sigma_item(kind, CS, HW, rng) for _ in range(n)]
    dev, host = [m[0] for m in made], [m[1] for m in made]
    var = capi.depth_sigma_batch(ws, dev, H, W, CS, capi.DEPTH_VARIANCE, pad=5)
    sig = capi.depth_sigma_batch(ws, dev, H, W, CS, capi.DEPTH_SIGMA, pad=5)
    var2 = capi.depth_sigma_batch(ws, dev, H, W, CS, capi.DEPTH_VARIANCE, pad=5)
    torch.cuda.synchronize()
    var, sig, var2 = var.cpu().numpy(), sig.cpu().numpy(), var2.cpu().numpy()
    assert np.isnan(var[:, HW:]).all() and np.isnan(sig[:, HW:]).all()       # the sentinels behind every map stay
    assert var.tobytes() == var2.tobytes()                                     # run to run: the same bytes
    N = 3 * (CS + 1) + 4
    worst, clamped = 0.0, 0
    for i, (bias, basis, code, scale, S) in enumerate(host):
        v64, mag = R.depth_variance(bias, basis, code, scale, S)
        err = np.abs(var[i, :HW].astype(np.float64) - v64)
        bound = R.gamma(N) * mag
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
        assert np.all(err <= bound)
        want = np.sqrt(np.maximum(var[i, :HW], np.float32(0.0)))              # fp32, correctly rounded
        assert np.all(np.abs(sig[i, :HW] - want) <= np.spacing(want))
        clamped += int(np.sum(var[i, :HW] < 0))
        assert np.all(sig[i, :HW][var[i, :HW] <= 0] == 0)
    print(f"depth variance CS {CS} HW {HW} n {n} {kind}: worst {worst:.3f} of gamma_{N} |j|'|S||j|; {clamped} pixels clamped")
    if (H, W, n) == (24, 32, 3):
        summary_line(f"depth variance CS {CS} 24x32 n 3 {kind}: worst {worst:.3f} of gamma_{N} |j|'|S||j|; {clamped} pixels clamped")


# ----------------------------------------------------------------------------------------- (g) sage_window_depth_sigma
@pytest.mark.parametrize("how", ["views", "prepared"])
@pytest.mark.parametrize("CS", [16, 32])
def test_window_depth_sigma(capi, ws, CS, how):
    import torch
    K = 4
    w = scene(K, CS)
    hold = {2: HOLD_CODE | HOLD_SCALE}
    prepared = None
    if how == "prepared":
        dks = [capi.DeviceKeyframe(kf, w.H, w.W) for kf in w.keyframes]
        prepared = dict(zip(range(K), capi.PreparedKeyframe.prepare_batch(ws, capi.prepare_config(w), dks)))
    win = capi.Window(w, holds=hold, prepared=prepared)
    st = capi.SageLmState(); st.damp = 1e-3
    cfg = capi.lm_config_default(); cfg.max_inner_evals = 1
    win.lm_step(st, cfg)                                                       # move the variables off their initial values
    win.linearize(); win.solve(0.0); win.covariance()
    kfs = [3, 0, 2]
    for mode in (capi.DEPTH_VARIANCE, capi.DEPTH_SIGMA):
        got = win.depth_sigma(kfs, mode)
        items = []
        for k in kfs:
            _pose, code, scale = win.get_keyframe(k)
            items.append((win.kfs[k].bias, win.kfs[k].basis, code, scale, win.get_covariance(k, k)[6:, 6:]))
        want = capi.depth_sigma_batch(ws, items, w.H, w.W, CS, mode)
        torch.cuda.synchronize()
        got, want = got.cpu().numpy().reshape(len(kfs), -1), want.cpu().numpy()
        assert got.tobytes() == want.tobytes()                                 # bit for bit
        assert not got[2].any()                                                # code and scale held: no depth variance
        assert np.all(got[0] > 0) and np.all(got[1] > 0)
    summary_line(f"window depth sigma CS {CS} ({how}): median sigma of keyframe 0 {float(np.median(got[1])):.3g}")
    win.close()
    for pk in (prepared or {}).values():
        pk.release()
