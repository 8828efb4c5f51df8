"""Matched-keypoint terms of the batched window engine (sage_window_add_keypoint_term) on the GPU: every term against the
fp32 oracle's per-edge operator, exact assembly into the packed system, reproducibility, error pass, solve, LM and sharding.
Tolerances are the project's own: TOL_H for per-edge AtA / Atb, 1e-5 for a per-edge error, 2e-6 for window totals, 1e-7 for
the engine's solve against the host block solve.  Next to the whole-matrix TOL_H every term goes entry by entry against the
fp64 oracle (tests/system_metric.py, families "window_reprojection" and "window_match_geometry": the code blocks of these terms are 1e-5
of the norm TOL_H is taken of)."""
import os
import socket

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import system_metric as sm
from tests.conftest import summary_line
from tests.helpers import prior_vectors, rel

pytestmark = pytest.mark.gpu

TOL_H = 2e-5
TOL_E = 1e-5
TOL_TOTAL = 2e-6
LOSSES = ("fair", "L2", "huber", "unbiased")


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


# (CS, match-geometry loss) of test_every_term_matches_the_oracle; tests/metric_cases.py measures the families' constants on
# the same terms
TERM_CASES = [(32, "fair"), (32, "L2"), (32, "huber"), (32, "unbiased"), (16, "fair")]


@pytest.fixture(scope="module", autouse=True)
def _metric_summary():
    yield
    for ln in sm.summary_lines("window keypoint terms"):
        summary_line(ln)


def make(CS=32):
    return synth.make_window(K=6, H=48, W=64, FS=16, CS=CS, L=3, n_samples=900, seed=5)


def edge_kfs(w, e):
    a, b = w.links[e // 2]
    return (a, b) if e % 2 == 0 else (b, a)


def rep_term(w, e, n=96, seed=0, **kw):
    k0, k1 = edge_kfs(w, e)
    t = synth.make_reprojection_matches(w, k0, k1, n, 1000 * seed + e, **kw)
    t.update(edge=e, weight=5.0, loss_param=0.1 * w.W * w.W)
    return t


def mg_term(w, e, loss, n=64, seed=0, **kw):
    k0, k1 = edge_kfs(w, e)
    t = synth.make_match_geometry_matches(w, k0, k1, n, 2000 * seed + e, **kw)
    t.update(edge=e, weight=5.0, loss=loss, loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
    return t


def all_terms(w, rep=True, mg_loss=None):
    """one reprojection term (N = 96) and / or one match-geometry term (N = 64) on every directed edge"""
    out = []
    for e in range(2 * len(w.links)):
        if rep:
            out.append(rep_term(w, e))
        if mg_loss is not None:
            out.append(mg_term(w, e, mg_loss))
    return out


def initial_vars(w):
    return [(kf.R, kf.t, kf.code, kf.scale) for kf in w.keyframes]


def engine_vars(win):
    out = []
    for k in range(win.K):
        pose, code, scale = win.get_keyframe(k)
        out.append((pose[:9].reshape(3, 3), pose[9:], code, scale))
    return out


def chunk_terms(w):
    """the terms of test_chunking_two_terms_on_one_edge_and_single_keypoint"""
    return [rep_term(w, 3, n=300), rep_term(w, 3, n=96, seed=1), rep_term(w, 4, n=1, outlier_share=1.0),
            mg_term(w, 7, "fair", n=300), mg_term(w, 8, "fair", n=1, outlier_share=1.0), rep_term(w, 0, n=64),
            rep_term(w, 1, n=65), mg_term(w, 2, "fair", n=128)]


def term_family(t):
    return "window_reprojection" if t["kind"] == "reprojection" else "window_match_geometry"


def oracle_term(orc, w, t, xs, jac=True, prec="f32"):
    k0, k1 = edge_kfs(w, t["edge"])
    (R0, t0, c0, s0), (R1, t1, c1, s1) = xs[k0], xs[k1]
    R0, t0, R1, t1 = (np.asarray(v, np.float32) for v in (R0, t0, R1, t1))
    R10, t10 = synth.relative_pose(R0, t0, R1, t1)
    a, b = w.keyframes[k0], w.keyframes[k1]
    if t["kind"] == "reprojection":
        if jac:
            return orc.reproj_jac_error(R10, t10, R0, t0, R1, t1, a.bias, a.basis, c0, t["loc0"], t["homo0"], t["matched_2d"],
                                        s0, w.cams[0], w.eps, t["loss_param"], t["weight"], prec=prec)
        e, n = orc.reproj_error(R10, t10, a.bias, a.basis, c0, t["loc0"], t["homo0"], t["matched_2d"], s0, w.cams[0], w.eps,
                                t["loss_param"], t["weight"])
        return dict(error=e, num_inliers=n)
    kw = dict(bias0=a.bias, bias1=b.bias, basis0=a.basis, basis1=b.basis, code0=c0, code1=c1, homo0=t["homo0"],
              homo1=t["homo1"], loc0=t["loc0"], loc1=t["loc1"], scale0=s0, scale1=s1, loss_param=t["loss_param"],
              weight=t["weight"])
    if jac:
        return orc.match_geom_jac_error(0, t["loss"], R10, t10, R0=R0, t0=t0, R1=R1, t1=t1, prec=prec, **kw)
    return dict(error=orc.match_geom_error(0, t["loss"], R10, t10, **kw))


def check_terms(orc, w, win, terms, label):
    xs = initial_vars(w)
    worst = dict(A=0.0, b=0.0, e=0.0)
    for i, t in enumerate(terms):
        h, o = win.get_keypoint_term(i), oracle_term(orc, w, t, xs)
        worst["A"] = max(worst["A"], rel(h["AtA"], o["AtA"]))
        worst["b"] = max(worst["b"], rel(h["Atb"], o["Atb"]))
        worst["e"] = max(worst["e"], abs(h["error"] - o["error"]) / abs(o["error"]))
        if t["kind"] == "reprojection":
            assert h["num_inliers"] == o["num_inliers"], (label, i)
        sm.check(h, oracle_term(orc, w, t, xs, prec="f64"), term_family(t), f"window term {label} #{i} edge {t['edge']}")
    summary_line(f"keypoint terms {label}: {len(terms)} terms, worst AtA {worst['A']:.2e} Atb {worst['b']:.2e} "
                 f"error {worst['e']:.2e}")
    assert worst["A"] < TOL_H and worst["b"] < TOL_H and worst["e"] < TOL_E, (label, worst)


# --------------------------------------------------------------------------------------------------------- 1. per term
@pytest.mark.parametrize("CS,loss", TERM_CASES)
def test_every_term_matches_the_oracle(capi, orc, CS, loss):
    w = make(CS)
    terms = all_terms(w, rep=True, mg_loss=loss)
    win = capi.Window(w, keypoint_terms=terms)
    assert win.num_keypoint_terms() == len(terms) == 4 * len(w.links)
    assert win.residuals_per_linearize == capi.Window(w).residuals_per_linearize + sum(
        (2 if t["kind"] == "reprojection" else 3) * len(t["loc0"]) for t in terms)
    win.linearize()
    check_terms(orc, w, win, terms, f"CS {CS} {loss}")
    win.close()


def test_chunking_two_terms_on_one_edge_and_single_keypoint(capi, orc):
    """N = 300 (several chunks, ragged last one), N = 1, and an edge that carries two reprojection terms.

    The single keypoint of the N = 1 terms is a gross mismatch (outlier_share = 1).  The robust error of ONE point,
    2 w sum_i (n_i - log(1 + n_i)), is a difference of nearly equal fp32 numbers when the residual is small: `1 + n_i` alone
    rounds by 6e-8, so the sum carries ~4e-7 of absolute rounding in ANY fp32 evaluation (the oracle's included: its N = 1
    term at 1 px noise sits 7e-6 from its own fp64 value), and the 1e-5 relative bar resolves it only where
    sum_i (n_i - log(1 + n_i)) >= ~0.1.  Terms of many points are dominated by their large residuals; for N = 1 the case is
    picked so, and the precondition is asserted on the oracle's value before the engine is compared."""
    w = make()
    terms = chunk_terms(w)
    for t in (terms[2], terms[4]):
        assert oracle_term(orc, w, t, initial_vars(w))["error"] / (2 * t["weight"]) >= 0.1
    win = capi.Window(w, keypoint_terms=terms)
    win.linearize()
    check_terms(orc, w, win, terms, "chunks")
    win.close()


def test_term_behind_the_camera_falls_back(capi, orc):
    """rays (x, y, -1): every point behind the camera -> no inliers, error = 10 * weight, zero blocks (a window of its own)"""
    w = make()
    t = rep_term(w, 2)
    t["homo0"] = (t["homo0"] * np.array([1, 1, -1], np.float32)).astype(np.float32)
    win = capi.Window(w, keypoint_terms=[t])
    win.linearize()
    h, o = win.get_keypoint_term(0), oracle_term(orc, w, t, initial_vars(w))
    assert o["num_inliers"] == 0 and h["num_inliers"] == 0
    assert h["error"] == pytest.approx(10 * t["weight"], rel=1e-6) and o["error"] == pytest.approx(10 * t["weight"], rel=1e-6)
    assert not h["AtA"].any() and not h["Atb"].any()
    dense = capi.Window(w)
    dense.linearize()
    a, b = win.packed_host(), dense.packed_host()
    assert np.array_equal(a[:-4], b[:-4]) and a[-4] + a[-3] == pytest.approx(b[-4] + b[-3] + 10 * t["weight"], rel=TOL_TOTAL)
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 2. assembly
def test_assembly_is_exact(capi):
    w = make()
    layers = [all_terms(w, rep=True, mg_loss="fair"), [rep_term(w, 5, n=96, seed=1), rep_term(w, 6, n=300, seed=1)]]
    terms = layers[0] + layers[1]
    win, dense = capi.Window(w, keypoint_terms=terms), capi.Window(w)
    win.linearize(); dense.linearize()
    a, b = win.packed_host(), dense.packed_host()
    got = a - b
    ref = np.zeros_like(a)
    i, err_sum = 0, 0.0
    for layer in layers:                                         # (the helper takes one result per (type, link, direction))
        res = {}
        for t in layer:
            key = (0 if t["kind"] == "reprojection" else 1, t["edge"] // 2, t["edge"] % 2)
            assert key not in res
            res[key] = win.get_keypoint_term(i)
            err_sum += float(res[key]["error"])
            i += 1
        ref += capi.assemble_packed(len(w.keyframes), w.links, w.CS, res)
    d = np.linalg.norm(got[:-4] - ref[:-4]) / np.linalg.norm(ref[:-4])
    summary_line(f"keypoint assembly: |with - without - assembled terms| / |assembled terms| = {d:.2e}; "
                 f"|dense| / |terms| = {np.linalg.norm(b[:-4]) / np.linalg.norm(ref[:-4]):.1e}")
    assert d < 1e-10
    assert a[-4] + a[-3] == pytest.approx(b[-4] + b[-3] + err_sum, rel=TOL_TOTAL)
    assert a[-4] - b[-4] == pytest.approx(ref[-4], rel=1e-5) and a[-3] - b[-3] == pytest.approx(ref[-3], rel=1e-5)
    assert np.array_equal(a[-2:], b[-2:])                        # the inlier slots stay dense-only
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 3. reproducible
def test_results_are_bit_reproducible(capi):
    w = make()
    terms = all_terms(w, rep=True, mg_loss="fair") + [rep_term(w, 3, n=300, seed=1)]
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


# --------------------------------------------------------------------------------------------------------- 4. error pass
def recomputed_total(capi, orc, w, terms, xs, dense):
    """dense engine's total (priors included) at variables xs + the oracle's keypoint errors there -> (total, keypoint part)"""
    for k, (R, t, code, scale) in enumerate(xs):
        dense.set_keyframe(k, capi.pack_pose(R, t), code, scale)
    dense.error(0)
    kp = sum(float(oracle_term(orc, w, t, xs, jac=False)["error"]) for t in terms)
    return dense.total_error(False) + kp, kp


@pytest.mark.parametrize("loss", LOSSES)
def test_error_pass_agrees_with_linearize_and_with_the_oracle(capi, orc, loss):
    w = make()
    terms = all_terms(w, rep=True, mg_loss=loss)
    win, dense = capi.Window(w, keypoint_terms=terms), capi.Window(w)
    win.linearize()
    e_lin = win.total_error(True)
    win.error(0)
    e_err = win.total_error(False)
    assert e_err == pytest.approx(e_lin, rel=TOL_TOTAL)
    # the linearize's own totals: dense engine + oracle
    ref0, kp0 = recomputed_total(capi, orc, w, terms, initial_vars(w), dense)
    assert abs(e_lin - ref0) <= TOL_TOTAL * ref0
    win.solve(1e-3)
    win.error(1)
    e_cand = win.total_error(False)
    win.accept()
    ref, kp = recomputed_total(capi, orc, w, terms, engine_vars(win), dense)
    summary_line(f"keypoint error pass ({loss}): candidate total {e_cand:.6f}, dense engine + oracle terms {ref:.6f} "
                 f"(terms {kp:.4f}), rel {abs(e_cand - ref) / ref:.2e}")
    assert abs(e_cand - ref) <= TOL_TOTAL * ref
    win.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 5. solve
@pytest.mark.parametrize("CS", [32, 16])
def test_solve_matches_host_block_solve(capi, CS):
    w = make(CS)
    K, B = len(w.keyframes), 7 + CS
    win = capi.Window(w, keypoint_terms=all_terms(w, rep=True, mg_loss="fair"))
    win.linearize()
    packed = win.packed_host().astype(np.float64)
    dadd, gadd = prior_vectors(w, CS)
    for damp in (1e-3, 1e-1):
        win.solve(damp)
        d = rel(win.delta(), capi.block_solve(packed[:-4], K, w.links, B, damp, dadd, gadd))
        summary_line(f"keypoint window CS {CS} damp {damp}: engine vs host block solve rel-L2 {d:.2e}")
        assert d < 1e-7
    win.close()


# --------------------------------------------------------------------------------------------------------- 6. LM
def lm_cfg(capi):
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    return cfg


def test_lm_step_descends_and_the_terms_reach_the_solve(capi):
    w = make()
    steps = {}
    for name, terms in (("dense", None), ("terms", all_terms(w, rep=True))):
        win = capi.Window(w, keypoint_terms=terms)
        st = capi.SageLmState(); st.damp = 1e-3
        win.lm_step(st, lm_cfg(capi))
        assert st.accepted == 1 and st.candidate_error < st.error, name
        steps[name] = win.delta().copy()
        win.close()
    d = rel(steps["terms"], steps["dense"])
    summary_line(f"keypoint LM: the reprojection terms move the damp 1e-3 step by {d:.3f} rel-L2")
    assert d > 1e-2
    win = capi.Window(w, keypoint_terms=all_terms(w, rep=True))
    st = capi.SageLmState(); st.damp = 1e-3
    tr = win.lm_run(st, lm_cfg(capi), 5)
    assert len(tr) == 5 and st.error < tr[0, 0]
    win.close()


def test_lm_with_match_geometry_never_ends_above_the_start(capi, orc):
    w = make()
    terms = all_terms(w, rep=True, mg_loss="fair")
    win, twin, dense = capi.Window(w, keypoint_terms=terms), capi.Window(w, keypoint_terms=terms), capi.Window(w)
    cfg = lm_cfg(capi)
    st = capi.SageLmState(); st.damp = 1e-3
    trace, checked = [], 0
    for _ in range(5):
        win.lm_step(st, cfg)
        trace.append((st.error, st.candidate_error, float(st.accepted), st.damp))
        if st.accepted:                                          # the candidate is the current estimate now: recompute it
            ref, kp = recomputed_total(capi, orc, w, terms, engine_vars(win), dense)
            assert abs(st.candidate_error - ref) <= TOL_TOTAL * ref
            checked += 1
    trace = np.array(trace)
    assert checked >= 1 and st.error <= trace[0, 0]
    st2 = capi.SageLmState(); st2.damp = 1e-3
    assert np.array_equal(twin.lm_run(st2, cfg, 5), trace)       # lm_run records the very same iterations
    summary_line(f"keypoint LM with match geometry: {trace[0, 0]:.3f} -> {st.error:.3f}, {checked} of 5 accepted")
    win.close(); twin.close(); dense.close()


# --------------------------------------------------------------------------------------------------------- 7. sharding
def test_two_shards_on_one_device_sum_to_the_single_rank_system(capi):
    w = make()
    terms = all_terms(w, rep=True, mg_loss="fair") + [rep_term(w, 5, n=300, seed=1)]
    one = capi.Window(w, keypoint_terms=terms)
    one.linearize()
    full = one.packed_host().copy()
    shards = [capi.Window(w, rank=r, world=2, keypoint_terms=terms) for r in range(2)]
    total = np.zeros_like(full)
    for sh in shards:
        assert sh.num_keypoint_terms() == len(terms)            # ids are global
        sh.linearize()
        total += sh.packed_host()
    assert np.linalg.norm(total - full) <= 1e-12 * np.linalg.norm(full)
    for i, t in enumerate(terms):
        rcs = [sh.get_keypoint_term(i, check=False)[0] for sh in shards]
        assert sorted(rc == 0 for rc in rcs) == [False, True], (i, rcs)
        owner = rcs.index(0)
        assert t["edge"] in capi.shard_edges(len(w.links), owner, 2)
        assert rcs[1 - owner] == -1                              # SAGE_E_INVALID, as sage_window_get_edge answers
        h, o = shards[owner].get_keypoint_term(i), one.get_keypoint_term(i)
        assert np.array_equal(h["AtA"], o["AtA"]) and h["error"] == o["error"]
    for sh in shards:
        sh.close()
    one.close()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run(win, capi, steps):
    cfg = lm_cfg(capi)
    cfg.linearize_at_candidate = -1
    st = capi.SageLmState()
    trace = []
    for _ in range(steps):
        win.lm_step(st, cfg)
        trace.append((st.error, st.candidate_error, int(st.accepted), st.damp))
    return np.array(trace)


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sage_slam_amd import capi
    w = make()
    win = capi.Window(w, rank=rank, world=world, keypoint_terms=all_terms(w, rep=True, mg_loss="fair"))
    win.set_allreduce(dist)
    np.save(os.path.join(out_dir, f"trace_{rank}.npy"), _run(win, capi, 4))
    np.save(os.path.join(out_dir, f"delta_{rank}.npy"), win.delta())
    dist.destroy_process_group()


def test_sharded_lm_step_with_terms_matches_single_rank(tmp_path):
    import torch.multiprocessing as mp
    from sage_slam_amd import capi
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    t0, t1 = (np.load(tmp_path / f"trace_{r}.npy") for r in range(world))
    assert np.array_equal(t0, t1)
    assert np.array_equal(np.load(tmp_path / "delta_0.npy"), np.load(tmp_path / "delta_1.npy"))
    w = make()
    single = _run(capi.Window(w, keypoint_terms=all_terms(w, rep=True, mg_loss="fair")), capi, 4)
    dense = _run(capi.Window(w), capi, 1)
    assert np.array_equal(single[:, 2], t0[:, 2])
    np.testing.assert_allclose(t0[:, :2], single[:, :2], rtol=1e-6)          # the tolerance of tests/test_gpu_sharded_lm.py
    assert abs(single[0, 0] - dense[0, 0]) > 1e-3 * dense[0, 0]              # (the terms are in these totals)


# --------------------------------------------------------------------------------------------------------- 8. misuse
def test_misuse_is_answered_with_status_codes(capi):
    w = make()
    good = rep_term(w, 0)
    for bad in (dict(good, edge=2 * len(w.links)), dict(good, edge=-1), dict(good, kind=5),
                dict(good, loc0=good["loc0"][:0], homo0=good["homo0"][:0], matched_2d=good["matched_2d"][:0]),
                dict(good, loc0=np.full_like(good["loc0"], w.H * w.W)), dict(mg_term(w, 0, "fair"), loss=9)):
        with pytest.raises(capi.SageError) as ei:
            capi.Window(w, keypoint_terms=[bad])
        assert ei.value.code == -1                               # SAGE_E_INVALID
    win = capi.Window(w, keypoint_terms=[good])
    assert win.add_keypoint_term(good) == -4                     # SAGE_E_STATE: after finalize
    assert win.num_keypoint_terms() == 1
    assert win.get_keypoint_term(0, check=False)[0] == -4        # nothing linearized yet
    assert win.get_keypoint_term(1, check=False)[0] == -1 and win.get_keypoint_term(-1, check=False)[0] == -1
    win.linearize()
    assert win.get_keypoint_term(0)["num_inliers"] == 96         # the window is still usable
    win.set_profiling(1)
    win.linearize(); win.error(0)
    assert win.kernel_time(4)[1] == 1 and win.kernel_time(5)[1] == 1         # one launch per pass for all terms
    win.close()
