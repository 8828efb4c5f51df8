"""Pose-graph terms of a window on the GPU (sage_window_add_graph_term): the relative-pose-scale, relative-pose and
scale-prior terms of the reference's live loop-closure graph (DeepFactors::LoopClosurePoseScaleEstimate) against the fp64
numpy restatement of tests/graph_term_ref.py, their assembly, their place next to dense factors and loop-MG terms, sharded
windows, and the graph itself solved as a window.

Per-term bars: 4 x the fp32 restatement's own distance from the fp64 one over the same terms, at least 2e-6, never above the
keypoint terms' 2e-5 / 2e-5 / 1e-5 (graph_term_ref.parity_bars).  The LM-delta bar is the project's 1e-4; the assembly bar
is the loop-graph test's 1e-10.  Term by term and entry by entry: dist_A / dist_b of tests/system_metric.py against the fp64
restatement under the "graph_terms" bars (measured: 3.6e-7 / 9.9e-6 against 2.1e-6 / 4.8e-5 over 203 terms).

Measured on an MI355X (summary_line prints the figures on every run; DESIGN.md s3 "Pose-graph terms of a window" quotes
them).  Per term, engine vs fp64 restatement, rel-L2 of AtA / Atb / error stacked over the terms of a window, next to the
fp32 restatement's own distance over the same terms:
    1 term 1.6e-7 / 5.5e-7 / 5.0e-7 (fp32 restatement 1.3e-7 / 2.1e-6 / 7.6e-7); 3, 4, 5, 15, 16, 17 and 53 terms
    <= 9.3e-8 / 6.8e-7 / 6.9e-7 (<= 7.9e-8 / 8.1e-7 / 6.0e-7); every theta, both directions, all kinds, CS 32 and 16:
    8.3e-8 / 6.5e-7 / 5.5e-7 (8.4e-8 / 6.4e-7 / 5.7e-7); next to dense factors and loop-MG terms 7.8e-8 / 2.7e-7 / 2.6e-7
    (9.8e-8 / 2.8e-7 / 2.6e-7).  Bars 2.0e-6 .. 8.5e-6.  On target: worst error 5.7e-4 of its bound.
Assembly |with - without - terms placed by hand| / |terms| = 3.1e-13; a reduced rank of two takes the single-rank first LM
step bit for bit (rel-L2 0.0).  The graph: first damped step vs a dense fp64 solve of the restated system 4.0e-7 (condition
number 1.3e2); recovery from 5.1e-2 / 7.4e-2 / 8.6e-2 (translation / relative scale / rotation) to 7.5e-9 / 5.0e-8 / 1.5e-7,
the fp64 numpy LM 9.0e-10 / 5.0e-8 / 3.9e-8 (7.5e-9 is one fp32 ulp of a translation coordinate: the window's variables are
fp32), error 0.5825 -> 1.3e-15; loop closure of a drifted chain: error 0.156683 -> 0.00239314 after 8 steps, the numpy LM
0.00239315 after 3."""
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import capi as capi_module                   # (pure-numpy helpers only; the library loads in the fixture)
from sage_slam_amd import synth
from tests import graph_term_ref as G
from tests import system_metric as sm
from tests.conftest import summary_line
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL_TOTAL = 2e-6
TERMS_PER_WAVE, TERMS_PER_BLOCK = 4, 16                          # graph_batch.h: 16 lanes a term, 256 threads a workgroup
INVALID, UNSUPPORTED, STATE = -1, -2, -4


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module", autouse=True)
def _metric_summary():
    yield
    for ln in sm.summary_lines("window graph terms"):
        summary_line(ln)


# --------------------------------------------------------------------------------------------------------- scenes
def base_window(CS=32, K=6):
    return synth.make_window(K=K, H=48, W=64, FS=16, CS=CS, L=3, n_samples=900, seed=5)


def theta_chain(CS=32):
    """K = 6 keyframes without a dense link whose consecutive relative rotations R_{k+1}^T R_k have the angles of G.THETAS
    (the first exactly the identity), unit-size translations, scales around 1; links (k, k + 1) and the chord (0, 5)"""
    w = base_window(CS, len(G.THETAS) + 1)
    rng = np.random.default_rng(21)
    pose = G.random_pose(rng)
    kfs = []
    for k, kf in enumerate(w.keyframes):
        if k > 0:
            axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
            th = G.THETAS[k - 1]
            R = pose[:9].reshape(3, 3) if th == 0.0 else pose[:9].reshape(3, 3) @ G.so3_exp(-th * axis)
            pose = np.concatenate([R.ravel(), rng.normal(0.0, 1.0, 3)])
        kfs.append(dataclasses.replace(kf, R=pose[:9].reshape(3, 3).astype(np.float32), t=pose[9:].astype(np.float32),
                                       scale=float(np.float32(rng.uniform(0.7, 1.4)))))
    links = [(k, k + 1) for k in range(len(kfs) - 1)] + [(0, len(kfs) - 1)]
    return dataclasses.replace(w, keyframes=kfs, links=[]), links


def variables(w):
    """what the engine holds: poses [K][12] and scales [K], fp32 values in fp64"""
    poses = [np.concatenate([kf.R.ravel(), kf.t]).astype(np.float32).astype(np.float64) for kf in w.keyframes]
    return poses, [float(np.float32(kf.scale)) for kf in w.keyframes]


def engine_variables(win):
    poses, scales = [], []
    for k in range(win.K):
        pose, _code, s = win.get_keyframe(k)
        poses.append(pose.astype(np.float64)); scales.append(float(s))
    return poses, scales


def term_on_edge(w, links, e, kind, rng, on_target=False):
    """a binary term on directed edge e whose target is 0.05 off the current relative pose and scales (or on them)"""
    poses, scales = variables(w)
    a, b = links[e // 2]
    k0, k1 = (a, b) if e % 2 == 0 else (b, a)
    if on_target:
        tgt, ts0, ts1 = G.relative_pose12(poses[k0], poses[k1]), scales[k0], scales[k1]
    else:
        tgt, ts0, ts1 = G.off_target(rng, poses[k0], poses[k1], scales[k0], scales[k1], kind)
    return dict(kind=kind, edge=e, target_pose10=tgt.astype(np.float32), target_scale0=float(np.float32(ts0)),
                target_scale1=float(np.float32(ts1)), weight=float(rng.uniform(0.5, 5.0)), rot_weight=float(rng.uniform(0.5, 2.0)),
                scale_weight=float(rng.uniform(1.0, 4.0)))


def n_terms(w, links, n, seed=0):
    """n terms that cycle over the directed edges (both directions, every theta) and the three kinds: terms repeat on edges"""
    rng = np.random.default_rng([seed, n])
    terms = []
    for i in range(n):
        kind = ("rel_pose_scale", "rel_pose", "scale_prior")[i % 3 if n >= 3 else 0]
        if kind == "scale_prior":
            kf = i % len(w.keyframes)
            terms.append(dict(kind=kind, kf=kf, target_scale0=float(np.float32(w.keyframes[kf].scale * np.exp(0.05))),
                              weight=float(rng.uniform(10.0, 100.0))))
        else:
            terms.append(term_on_edge(w, links, (5 * i) % (2 * len(links)), kind, rng))
    return terms


def cases_of(w, links, terms):
    poses, scales = variables(w)
    out = []
    for t in terms:
        k0, k1 = G.term_keyframes(t, links)
        out.append((t, poses[k0], poses[k1], scales[k0], scales[k1]))
    return out


def check_parity(win, w, links, terms, label):
    """the engine's per-term results against the fp64 restatement, stacked over the terms, under the bars of the same terms"""
    cases = cases_of(w, links, terms)
    ref = [G.linearize(*c) for c in cases]
    got = [win.get_graph_term(i) for i in range(len(terms))]
    bars, d32 = G.parity_bars(cases)
    stack = lambda rs, k: np.concatenate([np.ravel(np.asarray(r[k], np.float64)) for r in rs])
    dist = {k: G.rel_l2(stack(got, k), stack(ref, k)) for k in ("AtA", "Atb", "error")}
    fmt = lambda d: " / ".join(f"{d[k]:.1e}" for k in ("AtA", "Atb", "error"))
    summary_line(f"graph terms {label}: {len(terms)} terms, engine vs fp64 restatement (AtA / Atb / error) {fmt(dist)}, "
                 f"fp32 restatement {fmt(d32)}, bars {fmt(bars)}")
    for k in dist:
        assert dist[k] <= bars[k], (label, k, dist[k], bars[k])
    # ... and term by term, entry by entry (tests/system_metric.py): in the D = 14 layout the scale x scale entries are small
    # next to pose x pose, the stacked norms above are the pose blocks
    for i, (g, r) in enumerate(zip(got, ref)):
        sm.check(g, r, "graph_terms", f"{label} #{i} {terms[i]['kind']}", segs=sm.seg_loop(), against="the fp64 restatement")
    for t, g in zip(terms, got):                                 # columns a kind does not have read zero
        kind = G.kind_of(t)
        if kind == 1:
            assert not g["AtA"][12:].any() and not g["AtA"][:, 12:].any() and not g["Atb"][12:].any()
        if kind == 2:
            assert np.count_nonzero(g["AtA"]) == 1 and g["AtA"][12, 12] > 0 and not np.delete(g["Atb"], 12).any()
    return got, ref


# --------------------------------------------------------------------------------------------------------- 1. per term
COUNT_CASES = [1, TERMS_PER_WAVE - 1, TERMS_PER_WAVE, TERMS_PER_WAVE + 1,
               TERMS_PER_BLOCK - 1, TERMS_PER_BLOCK, TERMS_PER_BLOCK + 1, 3 * TERMS_PER_BLOCK + 5]


@pytest.mark.parametrize("n", COUNT_CASES)
def test_term_counts_around_a_wave_and_a_workgroup(capi, n):
    w, links = theta_chain()
    terms = n_terms(w, links, n)
    win = capi.Window(w, keypoint_links=links, graph_terms=terms)
    assert win.num_graph_terms() == n and win.num_keypoint_terms() == 0
    assert win.residuals_per_linearize == sum(G.ROWS[G.kind_of(t)] for t in terms)
    win.linearize()
    check_parity(win, w, links, terms, f"count {n}")
    win.close()


def every_theta_terms(w, links):
    """one off-target term of each binary kind on every directed edge, a scale prior on every keyframe -> (terms, the rng)"""
    rng = np.random.default_rng(3)
    terms = [term_on_edge(w, links, e, kind, rng) for e in range(2 * len(links)) for kind in ("rel_pose_scale", "rel_pose")]
    terms += [dict(kind="scale_prior", kf=k, target_scale0=float(np.float32(kf.scale * 1.05)), weight=100.0)
              for k, kf in enumerate(w.keyframes)]
    return terms, rng


def parity_term_sets():
    """every set of terms check_parity sees: [(label, window, links, terms)] (host side; tests/metric_cases.py measures the
    "graph_terms" constants of tests/system_metric.py on them)"""
    out = []
    for n in COUNT_CASES:
        w, links = theta_chain()
        out.append((f"count {n}", w, links, n_terms(w, links, n)))
    for CS in (32, 16):
        w, links = theta_chain(CS)
        out.append((f"every theta, CS {CS}", w, links, every_theta_terms(w, links)[0]))
    w = base_window()
    out.append(("on dense links", w, w.links, graph_on_dense(w)))
    return out


@pytest.mark.parametrize("CS", [32, 16])
def test_every_theta_both_directions_all_kinds(capi, CS):
    """every directed edge of the theta chain (relative rotations 0, 1e-4, 1e-2, 1, 2.5 and the chord's) carries one term of
    each binary kind, every keyframe a scale prior; then the same edges exactly on target"""
    w, links = theta_chain(CS)
    terms, rng = every_theta_terms(w, links)
    on = [term_on_edge(w, links, e, kind, rng, on_target=True) for e in range(2 * len(links)) for kind in ("rel_pose_scale", "rel_pose")]
    on += [dict(kind="scale_prior", kf=2, target_scale0=float(np.float32(w.keyframes[2].scale)), weight=100.0)]
    win = capi.Window(w, keypoint_links=links, graph_terms=terms + on)
    win.linearize()
    check_parity(win, w, links, terms, f"every theta, CS {CS}")
    worst = 0.0
    for i, t in enumerate(on):
        e = win.get_graph_term(len(terms) + i)["error"]
        worst = max(worst, e / G.on_target_bound(t))
        assert 0.0 <= e <= G.on_target_bound(t), (i, t["kind"], e)
    summary_line(f"graph terms on target, CS {CS}: worst error / (1e-10 w max(1, rot_w, scale_w)) = {worst:.2e}")
    # identity relative rotation (link 0: R0 = R1 bit for bit), target rotation the identity: the rotation residual is exactly
    # zero, so the rotation weight -- 1 or 1e10 -- changes no bit of the error or of the gradient
    eye = term_on_edge(w, links, 0, "rel_pose", rng)
    eye["target_pose10"][:9] = np.eye(3, dtype=np.float32).ravel()
    one = capi.Window(w, keypoint_links=links, graph_terms=[dict(eye, rot_weight=1.0), dict(eye, rot_weight=1.0e10)])
    one.linearize()
    g1, g2 = one.get_graph_term(0), one.get_graph_term(1)
    assert g1["error"] > 0 and g1["error"] == g2["error"] and np.array_equal(g1["Atb"], g2["Atb"])
    win.close(); one.close()


# --------------------------------------------------------------------------------------------------------- 2. assembly
def graph_on_dense(w, seed=4):
    """graph terms on the dense links of a window: both kinds on every directed edge, a second term on a few, two scale priors"""
    rng = np.random.default_rng(seed)
    E = 2 * len(w.links)
    terms = [term_on_edge(w, w.links, e, ("rel_pose_scale", "rel_pose")[e % 2], rng) for e in range(E)]
    terms += [term_on_edge(w, w.links, e, "rel_pose_scale", rng) for e in (0, 3, 3)]
    terms += [dict(kind="scale_prior", kf=k, target_scale0=float(np.float32(w.keyframes[k].scale * 1.1)), weight=50.0) for k in (0, 4)]
    return terms


def test_assembly_is_exact_touches_pose_and_scale_rows_only_and_repeats_bit_for_bit(capi):
    w = base_window()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    terms = graph_on_dense(w)
    win, dense = capi.Window(w, graph_terms=terms), capi.Window(w)
    win.linearize(); dense.linearize()
    a, b = win.packed_host().copy(), dense.packed_host()
    got = a - b
    res = [win.get_graph_term(i) for i in range(len(terms))]
    ref = G.assemble(K, w.links, CS, terms, res)
    d = np.linalg.norm(got[:-4] - ref[:-4]) / np.linalg.norm(ref[:-4])
    summary_line(f"graph-term assembly: |with - without - terms placed by hand| / |terms| = {d:.2e}")
    assert d < 1e-10
    H, g, _ = capi.unpack_dense(got, K, w.links, CS)
    code = [k * B + 6 + i for k in range(K) for i in range(CS)]
    assert not H[code, :].any() and not H[:, code].any() and not g[code].any()       # exactly 0
    assert a[-3] == pytest.approx(b[-3] + sum(float(r["error"]) for r in res), rel=TOL_TOTAL)   # the geometric error slot
    assert a[-4] == b[-4] and np.array_equal(a[-2:], b[-2:])                          # photometric slot, inlier slots
    win.linearize()
    assert np.array_equal(win.packed_host(), a)
    for i, r in enumerate(res):
        h = win.get_graph_term(i)
        assert np.array_equal(h["AtA"], r["AtA"]) and np.array_equal(h["Atb"], r["Atb"]) and h["error"] == r["error"]
    # a scale prior alone: one diagonal element, one gradient entry, its error
    prior = dict(kind="scale_prior", kf=3, target_scale0=float(np.float32(w.keyframes[3].scale * 1.2)), weight=100.0)
    one = capi.Window(w, graph_terms=[prior])
    one.linearize()
    diff = one.packed_host() - b
    r = one.get_graph_term(0)
    Hd, gd, tail = capi.unpack_dense(diff, K, w.links, CS)
    row = 3 * B + 6 + CS
    assert np.count_nonzero(Hd) == 1 and np.count_nonzero(gd) == 1
    assert Hd[row, row] == pytest.approx(float(r["AtA"][12, 12]), rel=1e-12) and gd[row] == pytest.approx(float(r["Atb"][12]), rel=1e-12)
    assert tail[1] == pytest.approx(float(r["error"]), rel=1e-6) and tail[0] == 0
    for x in (win, dense, one):
        x.close()


# --------------------------------------------------------------------------------------------------------- 3. mixed
def test_graph_terms_next_to_dense_factors_and_loop_mg_terms(capi):
    w = base_window()
    lmg = []
    for e in (0, 1, 4, 7):
        a, b = w.links[e // 2]
        k0, k1 = (a, b) if e % 2 == 0 else (b, a)
        t = synth.make_loop_mg_terms_from_matches(w, k0, k1, 64, 3000 + e)
        t.update(edge=e, weight=5.0, loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
        lmg.append(t)
    terms = graph_on_dense(w)
    win = capi.Window(w, keypoint_terms=lmg, graph_terms=terms)
    plain = capi.Window(w, keypoint_terms=lmg)
    assert win.residuals_per_linearize == plain.residuals_per_linearize + sum(G.ROWS[G.kind_of(t)] for t in terms)
    win.set_profiling(1)
    win.linearize(); plain.linearize()
    for e in range(2 * len(w.links)):                            # the dense per-edge results: bit-equal
        for type_ in (0, 1):
            h, o = win.get_edge(type_, e), plain.get_edge(type_, e)
            assert np.array_equal(h["AtA"], o["AtA"]) and np.array_equal(h["Atb"], o["Atb"]) and h["error"] == o["error"]
    for i in range(len(lmg)):                                    # ... and the loop-MG terms in front of them in the D = 14 buffers
        h, o = win.get_keypoint_term(i), plain.get_keypoint_term(i)
        assert np.array_equal(h["AtA"], o["AtA"]) and np.array_equal(h["Atb"], o["Atb"]) and h["error"] == o["error"]
    got, ref = check_parity(win, w, w.links, terms, "next to dense factors and loop-MG terms")
    restated = sum(float(r["error"]) for r in ref)
    e_with, e_without = win.total_error(True), plain.total_error(True)
    bars, _ = G.parity_bars(cases_of(w, w.links, terms))
    summary_line(f"mixed window: total error {e_with:.6f} = {e_without:.6f} (dense + loop-MG) + {e_with - e_without:.6f} "
                 f"(restated graph terms: {restated:.6f})")
    assert abs((e_with - e_without) - restated) <= bars["error"] * restated + 1e-12 * e_with
    win.error(0)
    assert win.total_error(False) == pytest.approx(e_with, rel=TOL_TOTAL)
    assert [win.kernel_time(k)[1] for k in (4, 5, 6, 7)] == [1, 1, 1, 1]   # one launch per pass for each family of terms
    win.close(); plain.close()


@pytest.mark.parametrize("CS", [32, 16])
def test_every_group_and_the_graph_terms_populated_at_once(capi, CS):
    """a four-keyframe window with its dense links, one reprojection, one match-geometry (N = 65: a full chunk and a remainder)
    and one loop-MG term, one graph term of each kind -- every group's buffers, the graph terms' place behind the loop-MG term
    and both runs of the {error, inliers} array are non-empty, so every offset of the layout is non-zero.  The kinds are added
    out of their layout order; the match-geometry and the loop-MG term, and the two binary graph terms, sit on one link in
    opposite directions.  Every term reads bit for bit what it reads on a window that holds it alone"""
    w = base_window(CS, K=4)
    rng = np.random.default_rng(11)
    kfs = lambda e: w.links[e // 2] if e % 2 == 0 else w.links[e // 2][::-1]
    bias2 = lambda e: float(0.1 * np.mean(np.square(w.keyframes[kfs(e)[0]].bias, dtype=np.float64)))
    lmg = synth.make_loop_mg_terms_from_matches(w, *kfs(3), 64, 3003)
    lmg.update(edge=3, weight=5.0, loss_param=bias2(3))
    rep = synth.make_reprojection_matches(w, *kfs(0), 40, 1000)
    rep.update(edge=0, weight=5.0, loss_param=0.1 * w.W * w.W)
    mg = synth.make_match_geometry_matches(w, *kfs(2), 65, 2002)
    mg.update(edge=2, weight=5.0, loss="fair", loss_param=bias2(2))
    kp = [lmg, rep, mg]
    gt = [dict(kind="scale_prior", kf=2, target_scale0=float(np.float32(w.keyframes[2].scale * 1.1)), weight=50.0),
          term_on_edge(w, w.links, 9, "rel_pose", rng), term_on_edge(w, w.links, 8, "rel_pose_scale", rng)]
    win, dense = capi.Window(w, keypoint_terms=kp, graph_terms=gt), capi.Window(w)
    win.linearize(); dense.linearize()
    a, b = win.packed_host().copy(), dense.packed_host()
    same = lambda h, o: all(np.array_equal(h[k], o[k]) for k in o)
    errs = []
    for i, t in enumerate(kp):
        alone = capi.Window(w, keypoint_terms=[t])
        alone.linearize()
        h, o = win.get_keypoint_term(i), alone.get_keypoint_term(0)
        assert set(o) == {"AtA", "Atb", "error", "num_inliers"} and same(h, o), ("keypoint term", i)
        assert o["AtA"].any() and o["error"] > 0
        errs.append((t["kind"], float(h["error"])))
        alone.close()
    for i, t in enumerate(gt):
        alone = capi.Window(w, graph_terms=[t])
        alone.linearize()
        h, o = win.get_graph_term(i), alone.get_graph_term(0)
        assert set(o) == {"AtA", "Atb", "error"} and same(h, o), ("graph term", i)
        assert o["AtA"].any() and o["error"] > 0
        errs.append((t["kind"], float(h["error"])))
        alone.close()
    photo = sum(e for kind, e in errs if kind == "reprojection")
    geo = sum(e for kind, e in errs if kind != "reprojection")
    assert a[-4] == pytest.approx(b[-4] + photo, rel=TOL_TOTAL) and a[-3] == pytest.approx(b[-3] + geo, rel=TOL_TOTAL)
    assert a[-4] > b[-4] and a[-3] > b[-3] and np.array_equal(a[-2:], b[-2:])       # the inlier slots stay dense-only
    e_lin = win.total_error(True)
    assert e_lin == pytest.approx(dense.total_error(True) + photo + geo, rel=TOL_TOTAL)
    win.error(0)
    assert win.total_error(False) == pytest.approx(e_lin, rel=TOL_TOTAL)
    win.linearize()
    assert np.array_equal(win.packed_host(), a)
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 4. sharding
def graph_only(capi, w, links, terms, **kw):
    return capi.Window(w, keypoint_links=links, graph_terms=terms, code_prior_weight=0.0, scale_prior_weight=0.0,
                       pose_prior_weight=0.0, **kw)


def small_graph():
    w = synth.make_window(K=6, H=48, W=64, FS=16, CS=32, L=3, n_samples=900, seed=5, loop_radius=0.08)
    K = len(w.keyframes)
    ring = [(min(k, (k + 1) % K), max(k, (k + 1) % K)) for k in range(K)]
    return synth.make_pose_graph(w, ring[:-1], loops=[ring[-1]], drift=0.01, seed=2)


def test_two_shards_on_one_device_sum_to_the_single_rank_system(capi):
    w, links, terms, holds = small_graph()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    one = graph_only(capi, w, links, terms, holds=holds)
    one.linearize()
    full = one.packed_host().copy()
    total = np.zeros_like(full)
    priors = [i for i, t in enumerate(terms) if t["kind"] == "scale_prior"]
    assert len(priors) == 3
    for r in range(2):
        sh = graph_only(capi, w, links, terms, holds=holds, rank=r, world=2)
        sh.linearize()
        total += sh.packed_host()
        for i in priors:                                         # a scale prior is rank 0's
            rc, _ = sh.get_graph_term(i, check=False)
            assert rc == (0 if r == 0 else INVALID)
        owned = capi.shard_edges(len(links), r, 2)
        for i, t in enumerate(terms):
            if t["kind"] != "scale_prior":
                assert sh.get_graph_term(i, check=False)[0] == (0 if t["edge"] in owned else INVALID)
        sh.close()
    assert np.linalg.norm(total - full) <= 1e-12 * np.linalg.norm(full)
    row = 6 + CS                                                 # contributed exactly once: keyframe 0's scale element
    d0 = lambda p: p[:K * B * B].reshape(K, B, B)[0][row, row]
    assert d0(total) == pytest.approx(d0(full), rel=1e-14)
    one.close()


class _NoPeers:
    """an all-reduce hook over one rank: the buffer stays as it is (the other rank's share comes from the emulation table)"""

    def all_reduce(self, t, group=None):
        pass


@pytest.mark.parametrize("rank", [0, 1])
def test_a_reduced_rank_with_emulated_peers_takes_the_single_rank_step(capi, rank):
    w, links, terms, holds = small_graph()
    one = graph_only(capi, w, links, terms, holds=holds)
    one.linearize()
    one.solve(1e-3)
    ref = one.delta().copy()
    sh = graph_only(capi, w, links, terms, holds=holds, rank=rank, world=2)
    other = graph_only(capi, w, links, terms, holds=holds, rank=1 - rank, world=2)
    other.linearize()
    rest = other.packed_tensor().clone().reshape(1, -1).contiguous()
    sh.set_allreduce(_NoPeers())
    sh.emulate_peers(rest)
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    st = capi.SageLmState(); st.damp = 1e-3
    sh.lm_step(st, cfg)
    d = rel(sh.delta(), ref)
    summary_line(f"reduced shard {rank} of 2 of a graph-term window: first LM delta vs the single-rank window's rel-L2 {d:.2e}")
    assert np.linalg.norm(ref) > 0
    assert np.array_equal(sh.delta(), ref)                       # bit for bit
    for win in (one, sh, other):
        win.close()


# --------------------------------------------------------------------------------------------------------- 5. the graph
def ring_and_chords(K):
    links = [(min(k, (k + 1) % K), max(k, (k + 1) % K)) for k in range(K)] + \
            [(min(k, (k + 2) % K), max(k, (k + 2) % K)) for k in range(K)]
    assert len(set(links)) == len(links)
    return links


def perturbed_scene(seed=5):
    """K = 8 keyframes around a circle, ring and chord links with EXACT targets; keyframes 1 .. K-1 start away from the truth
    as in tests/test_gpu_window_loop_graph.py graph_scene (pose by exp(N(0, 0.02^2)_6), scale by 1 + N(0, 0.05))"""
    K = 8
    w = synth.make_window(K=K, H=48, W=64, FS=16, CS=32, L=3, n_samples=900, seed=seed, loop_radius=0.08)
    rng = np.random.default_rng(1234)
    kfs = []
    for k, kf in enumerate(w.keyframes):
        R, t, s = kf.R_true.astype(np.float64), kf.t_true.astype(np.float64), float(kf.scale_true)
        if k > 0:
            d = rng.normal(0.0, 0.02, 6)
            dR = synth.so3_exp(d[3:])
            R, t, s = dR @ R, dR @ t + d[:3], s * (1.0 + rng.normal(0.0, 0.05))
        kfs.append(dataclasses.replace(kf, R=R.astype(np.float32), t=t.astype(np.float32), scale=float(np.float32(s))))
    w = dataclasses.replace(w, keyframes=kfs)
    return synth.make_pose_graph(w, ring_and_chords(K), local_targets="truth")


def free_rows(K, CS):
    """keyframe 0's pose and every code are held: the poses of keyframes 1 .. K-1 and all K scales are free"""
    B = 7 + CS
    return np.array([k * B + r for k in range(K) for r in (list(range(6)) if k > 0 else []) + [6 + CS]])


def restated_system(K, links, CS, terms, poses, scales):
    """the graph's system from the fp64 restatement at these variables -> (H, g, error)"""
    res = [G.linearize_on(t, links, poses, scales) for t in terms]
    H, g, _tail = capi_module.unpack_dense(G.assemble(K, links, CS, terms, res), K, links, CS)
    return H, g, sum(float(r["error"]) for r in res)


def restated_error(links, terms, poses, scales):
    return sum(float(G.error(t, poses[k0], poses[k1], scales[k0], scales[k1]))
               for t in terms for k0, k1 in [G.term_keyframes(t, links)])


def free_step(H, g, free, damp):
    Hf = H[np.ix_(free, free)]
    return np.linalg.solve(Hf + damp * np.diag(np.diag(Hf)), g[free])


def numpy_lm(K, links, CS, terms, poses, scales, iters, damp=1e-3, stop_rel=None):
    """LM in fp64 on the restated terms with the engine's policy as the tests configure it: one candidate per iteration,
    damp / 10 after an accepted step and * 10 after a rejected one, no clamp.  stop_rel: stop after an accepted step that
    lowers the error by less than that, relatively.  Variables and arithmetic are fp64 throughout"""
    B = 7 + CS
    free = free_rows(K, CS)
    poses, scales = [p.copy() for p in poses], list(scales)
    err = first = restated_error(links, terms, poses, scales)
    n = 0
    for n in range(1, iters + 1):
        H, g, _e = restated_system(K, links, CS, terms, poses, scales)
        delta = np.zeros(K * B)
        delta[free] = free_step(H, g, free, damp)
        cp = [G.retract(poses[k], delta[k * B:k * B + 6]) if k > 0 else poses[k] for k in range(K)]
        cs = [scales[k] + delta[k * B + 6 + CS] for k in range(K)]
        e = restated_error(links, terms, cp, cs)
        if e < err:
            gain = (err - e) / err
            poses, scales, err, damp = cp, cs, e, damp / 10
            if stop_rel is not None and gain < stop_rel:
                break
        else:
            damp *= 10
    return poses, scales, first, err, n


def truth_distances(w, poses, scales):
    """(max translation error, max relative scale error, max |R - R_true|_F) over the keyframes"""
    dt = max(float(np.linalg.norm(p[9:] - kf.t_true)) for p, kf in zip(poses, w.keyframes))
    ds = max(abs(s / kf.scale_true - 1.0) for s, kf in zip(scales, w.keyframes))
    dR = max(float(np.linalg.norm(p[:9].reshape(3, 3) - kf.R_true)) for p, kf in zip(poses, w.keyframes))
    return dt, ds, dR


def lm_config(capi):
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    cfg.damp_dec_factor = cfg.damp_inc_factor = 10.0
    cfg.min_damp, cfg.max_damp = 1e-30, 1e30                     # (the numpy schedule has no clamp)
    return cfg


def test_graph_first_step_and_recovery_of_the_truth(capi):
    """(a) the first damped step against a dense fp64 solve of the system assembled from the restatement; (b) LM from the
    perturbed start recovers the truth as an fp64 numpy LM on the restated terms does (at most ten times its distances);
    codes and keyframe 0's pose come out bit-equal to the start"""
    w, links, terms, holds = perturbed_scene()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    free = free_rows(K, CS)
    win = graph_only(capi, w, links, terms, holds=holds)
    assert win.Bs == 7
    p0, s0 = engine_variables(win)
    start_codes = [win.get_keyframe(k)[1].copy() for k in range(K)]
    # (a)
    win.linearize()
    win.solve(1e-3)
    delta = win.delta()
    held = np.setdiff1d(np.arange(K * B), free)
    assert np.all(delta[held] == 0.0)
    H, g, e_ref = restated_system(K, links, CS, terms, p0, s0)
    d = rel(delta[free], free_step(H, g, free, 1e-3))
    e_eng = win.total_error(True)
    summary_line(f"pose graph first step: vs dense fp64 solve of the restated system {d:.2e}; cond "
                 f"{np.linalg.cond(H[np.ix_(free, free)]):.1e}; error {e_eng:.6f} (restated {e_ref:.6f})")
    assert d <= 1e-4
    assert e_eng == pytest.approx(e_ref, rel=1e-5)
    # (b)
    iters = 15
    rp, rs, r_first, r_err, _ = numpy_lm(K, links, CS, terms, p0, s0, iters)
    st = capi.SageLmState(); st.damp = 1e-3
    tr = win.lm_run(st, lm_config(capi), iters)
    fp, fs = engine_variables(win)
    d0, de, dr = truth_distances(w, p0, s0), truth_distances(w, fp, fs), truth_distances(w, rp, rs)
    fmt = lambda v: " / ".join(f"{x:.1e}" for x in v)
    summary_line(f"pose graph recovery (translation / scale / rotation): start {fmt(d0)}, engine {fmt(de)}, numpy fp64 LM "
                 f"{fmt(dr)}; error {tr[0, 0]:.4f} -> {st.error:.2e} (numpy {r_first:.4f} -> {r_err:.2e}), "
                 f"{int(tr[:, 2].sum())} of {iters} accepted")
    for e, r in zip(de, dr):
        assert e <= 10 * r, (de, dr)
    for k in range(K):
        assert np.array_equal(win.get_keyframe(k)[1], start_codes[k])
    assert np.array_equal(fp[0], p0[0])                          # keyframe 0's pose: held
    win.close()


def test_loop_closure_of_a_drifted_chain(capi):
    """(c) a drifted chain whose local links sit on target plus one loop term whose target (the truth) disagrees with the
    chain: both LMs run until an accepted step lowers the error by less than 1e-6 relatively; the engine ends no higher than
    the numpy LM (x 1.001: parameter differences of 1e-4 move a quadratic minimum's value by ~1e-8)"""
    K = 8
    w0 = synth.make_window(K=K, H=48, W=64, FS=16, CS=32, L=3, n_samples=900, seed=5, loop_radius=0.08)
    chain = [(k, k + 1) for k in range(K - 1)]
    w, links, terms, holds = synth.make_pose_graph(w0, chain, loops=[(0, K - 1)], drift=0.01, seed=3)
    CS = w.CS
    win = graph_only(capi, w, links, terms, holds=holds)
    p0, s0 = engine_variables(win)
    cap = 60
    rp, rs, r_first, r_err, r_n = numpy_lm(K, links, CS, terms, p0, s0, cap, stop_rel=1e-6)
    cfg = lm_config(capi)
    st = capi.SageLmState(); st.damp = 1e-3
    win.linearize()
    e_eng = win.total_error(True)
    assert e_eng == pytest.approx(r_first, rel=1e-5)
    n = 0
    for n in range(1, cap + 1):
        win.lm_step(st, cfg)                                     # (st.error: at the iteration's start, st.candidate_error: after it)
        if st.accepted:
            gain, e_eng = (st.error - st.candidate_error) / st.error, st.candidate_error
            if gain < 1e-6:
                break
    fp, fs = engine_variables(win)
    e_at = restated_error(links, terms, fp, fs)
    summary_line(f"loop closure of a drifted chain: start error {r_first:.6f}; engine {e_eng:.8f} after {n} steps (restated at "
                 f"its variables {e_at:.8f}), numpy fp64 LM {r_err:.8f} after {r_n}")
    assert r_err < 0.5 * r_first                                 # the loop term does pull the chain
    assert e_eng <= r_err * (1 + 1e-3)
    assert e_at <= r_err * (1 + 1e-3)
    win.close()


# --------------------------------------------------------------------------------------------------------- 6. misuse
def test_misuse_is_answered_with_status_codes(capi, monkeypatch):
    w = base_window()
    rng = np.random.default_rng(0)
    good = term_on_edge(w, w.links, 1, "rel_pose_scale", rng)
    prior = dict(kind="scale_prior", kf=1, target_scale0=1.0, weight=10.0)
    nan_target = good["target_pose10"].copy(); nan_target[4] = np.nan
    inf_target = good["target_pose10"].copy(); inf_target[10] = np.inf
    for bad in (dict(good, edge=2 * len(w.links)), dict(good, edge=-1), dict(good, kind=3), dict(good, kind=-1),
                dict(good, weight=0.0), dict(good, weight=-1.0), dict(good, target_scale0=0.0), dict(good, target_scale1=-2.0),
                dict(good, target_pose10=nan_target), dict(good, target_pose10=inf_target), dict(good, target_scale0=float("nan")),
                dict(prior, kf=len(w.keyframes)), dict(prior, kf=-1), dict(prior, target_scale0=0.0), dict(prior, weight=0.0)):
        with pytest.raises(capi.SageError) as ei:
            capi.Window(w, graph_terms=[bad])
        assert ei.value.code == INVALID, bad
    win = capi.Window(w, graph_terms=[good, prior])
    assert win.add_graph_term(good) == STATE                     # after finalize
    assert win.num_graph_terms() == 2
    rc, _ = win.get_graph_term(0, check=False)
    assert rc == STATE                                           # before the first linearize
    assert win.get_graph_term(2, check=False)[0] == INVALID and win.get_graph_term(-1, check=False)[0] == INVALID
    win.linearize()                                              # the window is still usable
    assert win.get_graph_term(0)["AtA"].shape == (14, 14) and win.get_graph_term(1)["AtA"][12, 12] > 0
    win.solve(1e-3)
    win.close()
    # a window of the domain-decomposed solve knows no term on a single keyframe, and none of these
    monkeypatch.setenv("SAGE_SHARD_SCHUR", "1")
    with pytest.raises(capi.SageError) as ei:
        capi.Window(w, graph_terms=[good], rank=0, world=2)
    assert ei.value.code == UNSUPPORTED
    sh = capi.Window(w, rank=0, world=2)                         # ... without a term it finalizes as ever
    sh.linearize()
    sh.close()
    monkeypatch.delenv("SAGE_SHARD_SCHUR")
    ok = capi.Window(w, graph_terms=[good], rank=0, world=2)
    ok.linearize()
    ok.close()
