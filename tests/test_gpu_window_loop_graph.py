"""Loop-closure pose-scale graphs on the batched window engine, on the GPU: the loop-MG term kind (fixed depths, D = 14)
against the fp32 oracle, its exact assembly, links that carry keypoint terms only, windows without a dense edge, held variables,
and the pose-scale graph of DeepFactors::LoopClosurePoseScaleMGEstimate solved as a window like any other.
Tolerances are the project's own (tests/test_gpu_window_keypoints.py): TOL_H for per-term AtA / Atb, TOL_E for a per-term
error, TOL_TOTAL for window totals, 1e-7 for the engine's solve against the host block solve, 1e-4 for an LM delta against a
system assembled from the oracle's results.

Measured on an MI355X (summary_line prints the figures on every run; DESIGN.md s3 "Keypoint terms of a window" quotes them):
per term AtA <= 1.6e-7, Atb <= 3.7e-6, error <= 4.3e-7; graph recovery 1.0e-7 / 6.8e-8 / 2.0e-7 against the reference's
9.2e-8 / 5.0e-8 / 1.6e-7."""
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import synth
from tests.conftest import summary_line
from tests.helpers import prior_vectors, rel

pytestmark = pytest.mark.gpu

TOL_H = 2e-5
TOL_E = 1e-5
TOL_TOTAL = 2e-6
HOLD_CODE, HOLD_ALL = 2, 7                                       # SAGE_HOLD_CODE, all three


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


def make(CS=32, K=6):
    return synth.make_window(K=K, H=48, W=64, FS=16, CS=CS, L=3, n_samples=900, seed=5)


def edge_kfs(links, e):
    a, b = links[e // 2]
    return (a, b) if e % 2 == 0 else (b, a)


def loss_param_of(w, k0):
    return float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64)))


def lmg_term(w, links, e, n=64, seed=0, **kw):
    k0, k1 = edge_kfs(links, e)
    t = synth.make_loop_mg_terms_from_matches(w, k0, k1, n, 3000 * seed + e, **kw)
    t.update(edge=e, weight=5.0, loss_param=loss_param_of(w, k0))
    return t


def rep_term(w, links, e, n=96):
    k0, k1 = edge_kfs(links, e)
    t = synth.make_reprojection_matches(w, k0, k1, n, e)
    t.update(edge=e, weight=5.0, loss_param=0.1 * w.W * w.W)
    return t


def mg_term(w, links, e, n=64):
    k0, k1 = edge_kfs(links, e)
    t = synth.make_match_geometry_matches(w, k0, k1, n, 2000 + e)
    t.update(edge=e, weight=5.0, loss="fair", loss_param=loss_param_of(w, k0))
    return t


def initial_vars(w):
    return [(kf.R, kf.t, kf.code, kf.scale) for kf in w.keyframes]


def oracle_term(orc, w, links, t, xs, jac=True):
    """the oracle's per-edge operator for a term of any kind at variables xs"""
    k0, k1 = edge_kfs(links, t["edge"])
    (R0, t0, c0, s0), (R1, t1, c1, s1) = xs[k0], xs[k1]
    R0, t0, R1, t1 = (np.asarray(v, np.float32) for v in (R0, t0, R1, t1))
    R10, t10 = synth.relative_pose(R0, t0, R1, t1)
    a, b = w.keyframes[k0], w.keyframes[k1]
    if t["kind"] == "loop_mg":
        kw = dict(dpts0=t["u0"], dpts1=t["u1"], homo0=t["homo0"], homo1=t["homo1"], scale0=s0, scale1=s1,
                  loss_param=t["loss_param"], weight=t["weight"])
        if jac:
            return orc.match_geom_jac_error(1, "fair", R10, t10, R0=R0, t0=t0, R1=R1, t1=t1, **kw)
        return dict(error=orc.match_geom_error(1, "fair", R10, t10, **kw))
    if t["kind"] == "reprojection":
        return orc.reproj_jac_error(R10, t10, R0, t0, R1, t1, a.bias, a.basis, c0, t["loc0"], t["homo0"], t["matched_2d"], s0,
                                    w.cams[0], w.eps, t["loss_param"], t["weight"])
    return orc.match_geom_jac_error(0, t["loss"], R10, t10, R0=R0, t0=t0, R1=R1, t1=t1, bias0=a.bias, bias1=b.bias,
                                    basis0=a.basis, basis1=b.basis, code0=c0, code1=c1, homo0=t["homo0"], homo1=t["homo1"],
                                    loc0=t["loc0"], loc1=t["loc1"], scale0=s0, scale1=s1, loss_param=t["loss_param"],
                                    weight=t["weight"])


def check_terms(orc, w, win, terms, label):
    xs = initial_vars(w)
    worst = dict(A=0.0, b=0.0, e=0.0)
    for i, t in enumerate(terms):
        h, o = win.get_keypoint_term(i), oracle_term(orc, w, win.links, t, xs)
        assert h["AtA"].shape == o["AtA"].shape, (label, i)
        worst["A"] = max(worst["A"], rel(h["AtA"], o["AtA"]))
        worst["b"] = max(worst["b"], rel(h["Atb"], o["Atb"]))
        worst["e"] = max(worst["e"], abs(h["error"] - o["error"]) / abs(o["error"]))
        if t["kind"] != "reprojection":
            assert h["num_inliers"] == len(t["homo0"]), (label, i)
    summary_line(f"loop-graph terms {label}: {len(terms)} terms, worst AtA {worst['A']:.2e} Atb {worst['b']:.2e} "
                 f"error {worst['e']:.2e}")
    assert worst["A"] < TOL_H and worst["b"] < TOL_H and worst["e"] < TOL_E, (label, worst)


def sized_lmg_terms(orc, w, links):
    """loop-MG terms of N = 1 (a gross outlier), 64, 65 and 300 on four edges.  The N = 1 case as in
    tests/test_gpu_window_keypoints.py: the robust error of ONE point resolves the relative bar only where
    sum_i (n_i - log(1 + n_i)) >= ~0.1, which is asserted on the oracle's value before the engine is compared."""
    terms = [lmg_term(w, links, 1, n=1, seed=1, outlier_share=1.0), lmg_term(w, links, 2, n=64, seed=1),
             lmg_term(w, links, 3, n=65, seed=1), lmg_term(w, links, 4, n=300, seed=1)]
    assert oracle_term(orc, w, links, terms[0], initial_vars(w))["error"] / (2 * terms[0]["weight"]) >= 0.1
    return terms


def no_dense(w):
    """the window's keyframes without its links (they are added as keypoint links instead)"""
    return dataclasses.replace(w, links=[])


# --------------------------------------------------------------------------------------------------------- 1. per term
def test_all_three_kinds_in_one_window_match_the_oracle(capi, orc):
    """the largest dynamic-LDS size (match geometry present): every directed edge carries one term of each kind"""
    w = make()
    terms = []
    for e in range(2 * len(w.links)):
        terms += [rep_term(w, w.links, e), mg_term(w, w.links, e), lmg_term(w, w.links, e)]
    terms += sized_lmg_terms(orc, w, w.links)
    win = capi.Window(w, keypoint_terms=terms)
    assert win.residuals_per_linearize == capi.Window(w).residuals_per_linearize + sum(
        (2 if t["kind"] == "reprojection" else 3) * len(t["homo0"]) for t in terms)
    win.linearize()
    check_terms(orc, w, win, terms, "three kinds CS 32")
    win.close()


@pytest.mark.parametrize("CS", [32, 16])
def test_loop_mg_terms_alone_match_the_oracle(capi, orc, CS):
    """the smallest dynamic-LDS size (12 KB): loop-MG terms only"""
    w = make(CS)
    terms = [lmg_term(w, w.links, e) for e in range(2 * len(w.links))] + sized_lmg_terms(orc, w, w.links)
    win = capi.Window(w, keypoint_terms=terms)
    win.linearize()
    check_terms(orc, w, win, terms, f"loop-MG only CS {CS}")
    win.close()


# --------------------------------------------------------------------------------------------------------- 2. assembly
def test_assembly_is_exact_and_leaves_the_code_rows_alone(capi):
    w = make()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    terms = [lmg_term(w, w.links, e) for e in range(2 * len(w.links))]
    win, dense = capi.Window(w, keypoint_terms=terms), capi.Window(w)
    win.linearize(); dense.linearize()
    a, b = win.packed_host(), dense.packed_host()
    got = a - b
    res = {(2, t["edge"] // 2, t["edge"] % 2): win.get_keypoint_term(i) for i, t in enumerate(terms)}
    ref = capi.assemble_packed(K, w.links, CS, res)
    d = np.linalg.norm(got[:-4] - ref[:-4]) / np.linalg.norm(ref[:-4])
    summary_line(f"loop-MG assembly: |with - without - assembled terms| / |assembled terms| = {d:.2e}")
    assert d < 1e-10
    H, g, _ = capi.unpack_dense(got, K, w.links, CS)
    code = [k * B + 6 + i for k in range(K) for i in range(CS)]
    assert not H[code, :].any() and not H[:, code].any() and not g[code].any()       # exactly 0
    err_sum = sum(float(r["error"]) for r in res.values())
    assert a[-3] == pytest.approx(b[-3] + err_sum, rel=TOL_TOTAL)                     # the geometric error slot
    assert a[-4] == b[-4] and np.array_equal(a[-2:], b[-2:])                          # photometric slot, inlier slots
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 3. reproducible
def test_results_are_bit_reproducible(capi):
    w = make()
    terms = [lmg_term(w, w.links, e) for e in range(2 * len(w.links))] + [lmg_term(w, w.links, 3, n=300, seed=1),
                                                                         rep_term(w, w.links, 0), mg_term(w, w.links, 5)]
    w1, w2 = capi.Window(w, keypoint_terms=terms), capi.Window(w, keypoint_terms=terms)
    w1.linearize()
    p1 = w1.packed_host().copy()
    t1 = [w1.get_keypoint_term(i) for i in range(len(terms))]
    w1.linearize()
    w2.linearize()
    for win in (w1, w2):
        assert np.array_equal(win.packed_host(), p1)
        for i, ref in enumerate(t1):
            h = win.get_keypoint_term(i)
            assert np.array_equal(h["AtA"], ref["AtA"]) and np.array_equal(h["Atb"], ref["Atb"])
            assert h["error"] == ref["error"] and h["num_inliers"] == ref["num_inliers"]
    w1.error(0); e1 = w1.error_tensor().cpu().numpy().copy()
    w1.error(0); w2.error(0)
    assert np.array_equal(w1.error_tensor().cpu().numpy(), e1) and np.array_equal(w2.error_tensor().cpu().numpy(), e1)
    w1.close(); w2.close()


# --------------------------------------------------------------------------------------------------------- 4. keypoint links
def w1_terms(w, links):
    """the terms of window W1 (dense links + the loop closure 0 <-> K-1 as a keypoint link): loop-MG on both directions of
    the new link and on two dense edges, a match-geometry and a reprojection term on the new link as well"""
    e = 2 * (len(links) - 1)
    return [lmg_term(w, links, e), lmg_term(w, links, e + 1), lmg_term(w, links, 0), lmg_term(w, links, 7),
            mg_term(w, links, e), rep_term(w, links, e + 1)]


def term_key(t):
    return ({"reprojection": 0, "match_geometry": 1, "loop_mg": 2}[t["kind"]], t["edge"] // 2, t["edge"] % 2)


def test_a_keypoint_only_link_joins_the_system_and_leaves_the_dense_edges_alone(capi):
    import ctypes as C
    w = make()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    extra = (0, K - 1)
    assert extra not in w.links
    links = list(w.links) + [extra]
    terms = w1_terms(w, links)
    win = capi.Window(w, keypoint_links=[extra], keypoint_terms=terms)
    dense = capi.Window(w)
    assert win.nlinks == len(links) and win.links == links
    win.linearize(); dense.linearize()
    for e in range(2 * len(w.links)):                            # the dense per-edge results: bit-equal
        for type_ in (0, 1):
            h, o = win.get_edge(type_, e), dense.get_edge(type_, e)
            assert np.array_equal(h["AtA"], o["AtA"]) and np.array_equal(h["Atb"], o["Atb"]) and h["error"] == o["error"]
    e_new = 2 * (len(links) - 1)
    for e in (e_new, e_new + 1):
        for type_ in (0, 1):
            assert capi.lib().sage_window_get_edge(win.h, type_, e, None, None, None, None) == -1
    packed = win.packed_host().astype(np.float64)
    res = [(term_key(t), win.get_keypoint_term(i)) for i, t in enumerate(terms)]
    ref = np.zeros_like(packed)
    for key, r in res:                                           # (one result per (type, link, direction) and call)
        ref += capi.assemble_packed(K, links, CS, {key: r})
    blk = slice((K + len(links) - 1) * B * B, (K + len(links)) * B * B)
    assert np.linalg.norm(ref[blk]) > 0
    assert np.linalg.norm(packed[blk] - ref[blk]) <= 1e-12 * np.linalg.norm(ref[blk])
    dadd, gadd = prior_vectors(w, CS)
    for damp in (1e-3, 1e-1):
        win.solve(damp)
        d = rel(win.delta(), capi.block_solve(packed[:-4], K, links, B, damp, dadd, gadd))
        summary_line(f"window with a keypoint-only link, damp {damp}: engine vs host block solve rel-L2 {d:.2e}")
        assert d < 1e-7
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 5. no dense edge
def all_keypoint_window(capi, w, **kw):
    links = list(w.links)
    terms = [lmg_term(w, links, e) for e in range(2 * len(links))]
    return capi.Window(no_dense(w), keypoint_links=links, keypoint_terms=terms, **kw), terms


def test_a_window_without_a_dense_edge_linearizes_and_iterates(capi, orc):
    w = make()
    win, terms = all_keypoint_window(capi, w)                    # use_photo = use_geo = 1 left on
    assert win.nlinks == len(w.links) and win.residuals_per_linearize == 3 * 64 * len(terms)
    win.set_profiling(1)
    win.linearize()
    check_terms(orc, w, win, terms, "no dense edge")
    e_lin = win.total_error(True)
    win.error(0)
    assert win.total_error(False) == pytest.approx(e_lin, rel=TOL_TOTAL)
    tail = win.packed_host()[-4:]
    assert tail[0] == 0 and tail[2] == 0 and tail[3] == 0
    assert tail[1] == pytest.approx(sum(win.get_keypoint_term(i)["error"] for i in range(len(terms))), rel=TOL_TOTAL)
    assert [win.kernel_time(k)[1] for k in range(6)] == [0, 0, 0, 0, 1, 1]   # no dense kernel; one launch per pass for the terms
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    st = capi.SageLmState(); st.damp = 1e-3
    tr = win.lm_run(st, cfg, 5)
    assert len(tr) == 5 and np.isfinite(tr[:, 0]).all() and st.error <= tr[0, 0]
    assert all(win.kernel_time(k)[1] == 0 for k in range(4)) and win.kernel_time(4)[1] >= 1
    win.close()


# --------------------------------------------------------------------------------------------------------- 6. sharding
@pytest.mark.parametrize("which", ["W1", "keypoint links only"])
def test_two_shards_on_one_device_sum_to_the_single_rank_system(capi, which):
    w = make()
    if which == "W1":
        links = list(w.links) + [(0, len(w.keyframes) - 1)]
        build = lambda **kw: capi.Window(w, keypoint_links=links[-1:], keypoint_terms=w1_terms(w, links), **kw)
    else:
        build = lambda **kw: all_keypoint_window(capi, w, **kw)[0]
    one = build()
    one.linearize()
    full = one.packed_host().copy()
    total = np.zeros_like(full)
    for r in range(2):
        sh = build(rank=r, world=2)
        sh.linearize()
        total += sh.packed_host()
        sh.close()
    assert np.linalg.norm(total - full) <= 1e-12 * np.linalg.norm(full)
    one.close()


class _NoPeers:
    """an all-reduce hook over one rank: the buffer stays as it is (the other rank's share comes from the emulation table)"""

    def all_reduce(self, t, group=None):
        pass


@pytest.mark.parametrize("rank", [0, 1])
def test_a_reduced_shard_assembles_the_link_blocks_only_its_terms_write(capi, rank):
    """One rank of a two-rank window without a dense edge, the other rank's share from sage_window_emulate_peers: the LM
    iteration of a reduced window assembles only the blocks this rank contributes to.  A link block that only local TERMS
    write to must be among them -- the step it takes then is the single-rank window's."""
    w = make()
    one, _ = all_keypoint_window(capi, w)
    one.linearize()
    one.solve(1e-3)
    ref = one.delta().copy()
    sh, _ = all_keypoint_window(capi, w, rank=rank, world=2)
    other, _ = all_keypoint_window(capi, w, rank=1 - rank, world=2)
    other.linearize()
    rest = other.packed_tensor().clone().reshape(1, -1).contiguous()
    sh.set_allreduce(_NoPeers())
    sh.emulate_peers(rest)
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    st = capi.SageLmState(); st.damp = 1e-3
    sh.lm_step(st, cfg)
    d = rel(sh.delta(), ref)
    summary_line(f"reduced shard {rank} of 2 without a dense edge: first LM delta vs the single-rank window's rel-L2 {d:.2e}")
    assert d < 1e-7
    for win in (one, sh, other):
        win.close()


# --------------------------------------------------------------------------------------------------------- 7. holds
def held_rows(holds, K, CS):
    B = 7 + CS
    rows = []
    for k, m in holds.items():
        rows += [k * B + r for r in range(6)] if m & 1 else []
        rows += [k * B + 6 + i for i in range(CS)] if m & 2 else []
        rows += [k * B + 6 + CS] if m & 4 else []
    return sorted(rows)


def masked_system(packed, dadd, gadd, K, links, CS, holds):
    """the held rule on a host copy: held rows / columns zeroed in diagonal and link blocks, unit diagonal, zero right-hand
    side, no priors on held rows"""
    B = 7 + CS
    BB = B * B
    p = packed.copy(); dadd = dadd.copy(); gadd = gadd.copy()
    diag = p[:K * BB].reshape(K, B, B)
    lnk = p[K * BB:(K + len(links)) * BB].reshape(len(links), B, B)
    g = p[(K + len(links)) * BB:(K + len(links)) * BB + K * B].reshape(K, B)
    for idx in held_rows(holds, K, CS):
        k, r = divmod(idx, B)
        diag[k][r, :] = 0; diag[k][:, r] = 0; diag[k][r, r] = 1
        g[k][r] = 0; dadd[idx] = 0; gadd[idx] = 0
        for l, (a, b) in enumerate(links):
            if a == k:
                lnk[l][r, :] = 0
            if b == k:
                lnk[l][:, r] = 0
    return p, dadd, gadd


def all_vars(win):
    return [win.get_keyframe(k) for k in range(win.K)]


def test_held_variables_stay_put_and_the_free_ones_see_them_eliminated(capi):
    w = make()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    assert np.array_equal(w.keyframes[0].R, np.eye(3, dtype=np.float32))           # exact zeros among the held entries
    holds = {0: HOLD_ALL, 1: HOLD_ALL, 2: capi.SAGE_HOLD_CODE}
    win = capi.Window(w, holds=holds)
    win.linearize()
    packed = win.packed_host().astype(np.float64)
    plain = capi.Window(w)
    plain.linearize()
    assert np.array_equal(packed, plain.packed_host())                              # the packed buffer is untouched by holds
    dadd, gadd = prior_vectors(w, CS)
    held = held_rows(holds, K, CS)
    free = np.setdiff1d(np.arange(K * B), held)
    pm, dm, gm = masked_system(packed[:-4], dadd, gadd, K, w.links, CS, holds)
    for damp in (1e-3, 1e-1):
        win.solve(damp)
        delta = win.delta()
        assert np.all(delta[held] == 0.0)
        ref = capi.block_solve(pm, K, w.links, B, damp, dm, gm)
        d = rel(delta[free], ref[free])
        summary_line(f"held window damp {damp}: free entries vs host block solve of the masked system rel-L2 {d:.2e}")
        assert d < 1e-7 and np.abs(ref[held]).max() == 0.0
        plain.solve(damp)
        assert rel(delta[free], plain.delta()[free]) > 1e-3                         # (the holds do change the step)
    win.accept()
    for k, m in holds.items():
        pose, code, scale = win.get_keyframe(k)
        kf = w.keyframes[k]
        if m & 1:
            assert np.array_equal(pose, np.concatenate([kf.R.ravel(), kf.t]).astype(np.float32))
        if m & 2:
            assert np.array_equal(code, kf.code)
        if m & 4:
            assert scale == np.float32(kf.scale)
    pose3, code3, scale3 = win.get_keyframe(3)
    assert not np.array_equal(code3, w.keyframes[3].code) and not np.array_equal(pose3[9:], w.keyframes[3].t)
    win.close(); plain.close()


def test_zero_masks_change_no_bit(capi):
    w = make()
    a, b = capi.Window(w), capi.Window(w, holds={k: 0 for k in range(len(w.keyframes))})
    for win in (a, b):
        win.linearize()
        win.solve(1e-3)
    assert np.array_equal(a.packed_host(), b.packed_host()) and np.array_equal(a.delta(), b.delta())
    for win in (a, b):
        win.accept()
    for (pa, ca, sa), (pb, cb, sb) in zip(all_vars(a), all_vars(b)):
        assert np.array_equal(pa, pb) and np.array_equal(ca, cb) and sa == sb
    a.close(); b.close()


# --------------------------------------------------------------------------------------------------------- 8. the graph
def graph_scene(seed=5):
    """K = 8 keyframes around a circle; ring and chord links; keyframes 1 .. K-1 start away from the truth (pose by
    exp(N(0, 0.02^2)_6), scale by 1 + N(0, 0.05)), keyframe 0 at it"""
    K = 8
    w = synth.make_window(K=K, H=48, W=64, FS=16, CS=32, L=3, n_samples=900, seed=seed, loop_radius=0.08)
    links = [(min(k, (k + 1) % K), max(k, (k + 1) % K)) for k in range(K)] + \
            [(min(k, (k + 2) % K), max(k, (k + 2) % K)) for k in range(K)]
    assert len(set(links)) == len(links)
    rng = np.random.default_rng(1234)
    kfs = []
    for k, kf in enumerate(w.keyframes):
        R, t, s = kf.R_true.astype(np.float64), kf.t_true.astype(np.float64), float(kf.scale_true)
        if k > 0:
            d = rng.normal(0.0, 0.02, 6)
            dR = synth.so3_exp(d[3:])
            R, t, s = dR @ R, dR @ t + d[:3], s * (1.0 + rng.normal(0.0, 0.05))
        kfs.append(dataclasses.replace(kf, R=R.astype(np.float32), t=t.astype(np.float32), scale=float(np.float32(s))))
    w = dataclasses.replace(w, keyframes=kfs, links=[])
    terms = []
    for l, (a, b) in enumerate(links):
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            t = synth.make_loop_mg_exact(w, k0, k1, 64, 7)
            t.update(edge=2 * l + d, weight=5.0, loss_param=loss_param_of(w, k0))
            terms.append(t)
    holds = {k: HOLD_CODE for k in range(K)}
    holds[0] = HOLD_ALL
    return w, links, terms, holds


def graph_free_rows(K, CS):
    B = 7 + CS
    return np.array([k * B + r for k in range(1, K) for r in list(range(6)) + [6 + CS]])


def oracle_system(orc, capi, w, links, terms, xs):
    """the packed system of the graph from the oracle's per-term results at variables xs -> (H, g, error)"""
    res = {term_key(t): oracle_term(orc, w, links, t, xs) for t in terms}
    for r in res.values():
        r["num_inliers"] = 0
    H, g, tail = capi.unpack_dense(capi.assemble_packed(len(w.keyframes), links, w.CS, res), len(w.keyframes), links, w.CS)
    return H, g, tail[1]


def free_step(H, g, free, damp):
    Hf = H[np.ix_(free, free)]
    return np.linalg.solve(Hf + damp * np.diag(np.diag(Hf)), g[free])


def distances(w, xs):
    """(max translation error, max relative scale error, max |R - R_true|_F) over the keyframes"""
    dt = max(float(np.linalg.norm(np.asarray(t, np.float64) - kf.t_true)) for (R, t, c, s), kf in zip(xs, w.keyframes))
    ds = max(abs(float(s) / kf.scale_true - 1.0) for (R, t, c, s), kf in zip(xs, w.keyframes))
    dR = max(float(np.linalg.norm(np.asarray(R, np.float64).reshape(3, 3) - kf.R_true)) for (R, t, c, s), kf in zip(xs, w.keyframes))
    return dt, ds, dR


def engine_vars(win):
    out = []
    for k in range(win.K):
        pose, code, scale = win.get_keyframe(k)
        out.append((pose[:9].reshape(3, 3), pose[9:], code, scale))
    return out


def reference_lm(orc, capi, w, links, terms, iters=12, damp=1e-3):
    """the reference LM on the oracle's terms: dense solve on the free rows, damp / 10 on accept and * 10 on reject"""
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    free = graph_free_rows(K, CS)
    xs = initial_vars(w)
    total = lambda v: sum(oracle_term(orc, w, links, t, v, jac=False)["error"] for t in terms)
    err = first = total(xs)
    for _ in range(iters):
        H, g, _e = oracle_system(orc, capi, w, links, terms, xs)
        delta = np.zeros(K * B)
        delta[free] = free_step(H, g, free, damp)
        cand = [xs[0]]
        for k in range(1, K):
            R, t, c, s = xs[k]
            pose = capi.pose_retract(np.concatenate([np.asarray(R, np.float32).ravel(), np.asarray(t, np.float32)]),
                                     delta[k * B:k * B + 6].astype(np.float32))
            cand.append((pose[:9].reshape(3, 3), pose[9:], c, float(np.float32(s) + np.float32(delta[k * B + 6 + CS]))))
        e = total(cand)
        if e < err:
            xs, err, damp = cand, e, damp / 10
        else:
            damp *= 10
    return xs, first, err


def test_pose_scale_graph_first_step_and_recovery(capi, orc):
    """(a) the first damped step against a dense solve of the engine's own system and of the oracle-assembled one on the
    free pose / scale rows; (b) twelve LM steps recover the true poses and scales as the reference LM on the oracle's terms
    does (at most ten times its distance, or 1e-6: both sit at their fp32 rounding floor, in different summation orders)."""
    w, links, terms, holds = graph_scene()
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    free = graph_free_rows(K, CS)
    win = capi.Window(w, keypoint_links=links, keypoint_terms=terms, holds=holds, code_prior_weight=0.0)
    start = engine_vars(win)
    # (a)
    win.linearize()
    H, g, tail = capi.unpack_dense(win.packed_host().astype(np.float64), K, links, CS)
    win.solve(1e-3)
    delta = win.delta()
    held = np.setdiff1d(np.arange(K * B), free)
    assert np.all(delta[held] == 0.0)
    d_own = rel(delta[free], free_step(H, g, free, 1e-3))
    Ho, go, eo = oracle_system(orc, capi, w, links, terms, initial_vars(w))
    d_orc = rel(delta[free], free_step(Ho, go, free, 1e-3))
    summary_line(f"pose-scale graph first step: vs dense solve of the engine's system {d_own:.2e}, of the oracle's {d_orc:.2e}; "
                 f"cond {np.linalg.cond(H[np.ix_(free, free)]):.1e}; error {tail[1]:.4f} (oracle {eo:.4f})")
    assert d_own < 1e-7 and d_orc < 1e-4
    # (b)
    ref_xs, ref_first, ref_err = reference_lm(orc, capi, w, links, terms)
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    cfg.damp_dec_factor = cfg.damp_inc_factor = 10.0
    cfg.min_damp, cfg.max_damp = 1e-30, 1e30                     # (the reference schedule has no clamp)
    st = capi.SageLmState(); st.damp = 1e-3
    tr = win.lm_run(st, cfg, 12)
    final = engine_vars(win)
    d0, de, dr = distances(w, start), distances(w, final), distances(w, ref_xs)
    fmt = lambda d: " / ".join(f"{v:.1e}" for v in d)
    summary_line(f"pose-scale graph recovery (translation / scale / rotation): start {fmt(d0)}, engine {fmt(de)}, "
                 f"reference {fmt(dr)}; error {tr[0, 0]:.3f} -> {st.error:.2e} (reference {ref_first:.3f} -> {ref_err:.2e}), "
                 f"{int(tr[:, 2].sum())} of 12 accepted")
    for e, r in zip(de, dr):
        assert e <= max(10 * r, 1e-6), (de, dr)
    for k in range(K):                                           # codes and keyframe 0: bit-equal to the start
        assert np.array_equal(final[k][2], start[k][2])
    assert np.array_equal(final[0][0], start[0][0]) and np.array_equal(final[0][1], start[0][1]) and final[0][3] == start[0][3]
    assert st.error <= 1e-6 * tr[0, 0]
    win.close()


# --------------------------------------------------------------------------------------------------------- 9. misuse
def test_misuse_is_answered_with_status_codes(capi):
    w = make()
    K = len(w.keyframes)
    good = lmg_term(w, w.links, 0)
    for bad in (dict(good, u0=None), dict(good, u1=None), dict(good, homo1=None), dict(good, loss_param=0.0),
                dict(good, loss_param=-1.0), dict(good, edge=2 * len(w.links))):
        with pytest.raises(capi.SageError) as ei:
            capi.Window(w, keypoint_terms=[bad])
        assert ei.value.code == -1                               # SAGE_E_INVALID
    for holds in ({K: 1}, {-1: 1}, {0: 8}, {0: -1}):
        with pytest.raises(capi.SageError) as ei:
            capi.Window(w, holds=holds)
        assert ei.value.code == -1
    for link in ((0, 0), (0, K), (-1, 1)):
        with pytest.raises(capi.SageError) as ei:
            capi.Window(w, keypoint_links=[link])
        assert ei.value.code == -1
    # a term on the keypoint link's edge is fine, one beyond 2 * nlinks is not
    extra = (0, K - 1)
    links = list(w.links) + [extra]
    on_new = lmg_term(w, links, 2 * len(w.links) + 1)
    with pytest.raises(capi.SageError) as ei:
        capi.Window(w, keypoint_links=[extra], keypoint_terms=[dict(on_new, edge=2 * len(links))])
    assert ei.value.code == -1
    win = capi.Window(w, keypoint_links=[extra], keypoint_terms=[on_new], holds={1: capi.SAGE_HOLD_SCALE})
    assert win.hold(0, 1) == -4 and win.add_keypoint_link(1, 4) == -4          # SAGE_E_STATE: after finalize
    assert win.nlinks == len(links) and capi.lib().sage_window_num_links(win.h) == len(links)
    assert win.add_keypoint_term(on_new) == -4
    win.linearize()                                              # the window is still usable
    assert win.get_keypoint_term(0)["num_inliers"] == 64 and win.get_keypoint_term(0)["AtA"].shape == (14, 14)
    win.solve(1e-3)
    assert win.delta()[1 * (7 + w.CS) + 6 + w.CS] == 0.0
    win.close()
