"""Solver rows on the GPU: a window in which every keyframe holds a whole variable group (pose, code or scale) solves a
damped system of the remaining groups only (sage_window_solver_block_size; sage_slam_amd/csrc/window_plan.h: solver_rows) --
the device scatter writes blocks of the kept rows, the host factorises them, the retract reads the solution through the row
map; windows with duplicate links do the same on the host.  The step is the one the identity-row system gave: the bars are
those of tests/test_gpu_window_loop_graph.py (1e-7 against the host block solve of the masked system and against a dense
solve of the free rows of the engine's own system; the acceptance rule of the pose-scale graph's recovery).

Shapes as there: K = 6 / 8 keyframes at 48 x 64, CS = 32, loop-MG terms of 64 points.

Measured on an MI355X (summary_line prints the figures on every run; DESIGN.md s3 "Solver rows" quotes them): free rows vs
the host block solve of the masked system 0.0 (Bs = 7, 6) and 1.1e-8 / 3.5e-10 (Bs = 33, damp 1e-3 / 1e-1), vs a dense solve
of the engine's free rows <= 8.7e-14 (Bs = 7, 6) and 1.1e-8 / 3.5e-10 (Bs = 33); all codes held moves the pose / scale step by
1.3 / 0.43; recovery 9.3e-8 / 6.8e-8 / 1.9e-7 against the reference's 9.2e-8 / 5.0e-8 / 1.6e-7."""
import dataclasses

import numpy as np
import pytest

from tests.conftest import summary_line
from tests.helpers import prior_vectors, rel
from tests.test_gpu_window_loop_graph import (_NoPeers, all_keypoint_window, distances, engine_vars, graph_scene, held_rows,
                                              make, masked_system, reference_lm)

pytestmark = pytest.mark.gpu

POSE, CODE, SCALE, ALL = 1, 2, 4, 7


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


def dense_case(capi, mask, **kw):
    """the dense window of the loop-graph tests with `mask` held on every keyframe -> (window data, links, Window, holds,
    code prior weight)"""
    w = make()
    holds = {k: mask for k in range(len(w.keyframes))}
    return w, list(w.links), capi.Window(w, holds=holds, **kw), holds, 1e-3


def graph_case(capi):
    w, links, terms, holds = graph_scene()
    return w, links, capi.Window(w, keypoint_links=links, keypoint_terms=terms, holds=holds, code_prior_weight=0.0), holds, 0.0


def duplicate_case(capi):
    """a dense link added twice: no device solver, the window solves on the host"""
    w = make()
    w = dataclasses.replace(w, links=list(w.links) + [w.links[1]])
    holds = {k: CODE for k in range(len(w.keyframes))}
    return w, list(w.links), capi.Window(w, holds=holds), holds, 1e-3


CASES = {"pose-scale graph": (graph_case, 7), "all codes": (lambda c: dense_case(c, CODE), 7),
         "all codes and scales": (lambda c: dense_case(c, CODE | SCALE), 6), "all poses": (lambda c: dense_case(c, POSE), 33),
         "all codes, duplicate link": (duplicate_case, 7)}


# ------------------------------------------------------------------------------------------------------ 1. block sizes
def test_solver_block_sizes(capi):
    L = capi.lib()
    CS = 32
    B = 7 + CS
    for name, (build, Bs) in CASES.items():
        w, links, win, holds, _ = build(capi)
        K = len(w.keyframes)
        assert L.sage_window_solver_block_size(win.h) == Bs and win.Bs == Bs, name
        assert L.sage_window_block_size(win.h) == B and win.B == B, name
        assert win.packed_count == (K + len(links)) * B * B + K * B + 4, name
        win.close()
    w = make()
    K = len(w.keyframes)
    one_free = {k: CODE for k in range(K)}
    one_free[3] = 0
    for holds in (None, one_free, {k: ALL for k in range(K)}):     # nothing held; one free code; nothing left to solve for
        win = capi.Window(w, holds=holds)
        assert win.Bs == B and win.B == B and win.packed_count == (K + len(w.links)) * B * B + K * B + 4
        win.close()


# ------------------------------------------------------------------------------------------------------ 2. / 4. the step
@pytest.mark.parametrize("name", list(CASES))
def test_the_compact_solve_takes_the_step_of_the_masked_system(capi, name):
    build, Bs = CASES[name]
    w, links, win, holds, code_w = build(capi)
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    assert win.Bs == Bs
    start = [win.get_keyframe(k) for k in range(K)]
    win.linearize()
    packed = win.packed_host().astype(np.float64)
    dadd, gadd = prior_vectors(w, CS, code_w=code_w)
    held = held_rows(holds, K, CS)
    free = np.setdiff1d(np.arange(K * B), held)
    assert len(free) and len(free) <= K * Bs
    pm, dm, gm = masked_system(packed[:-4], dadd, gadd, K, links, CS, holds)
    H, g, _ = capi.unpack_dense(packed, K, links, CS)
    Hf = H[np.ix_(free, free)] + np.diag(dadd[free])
    for damp in (1e-3, 1e-1):
        win.solve(damp)
        delta = win.delta()
        assert np.all(delta[held] == 0.0) and not np.signbit(delta[held]).any()      # exactly 0.0 on dropped and held rows
        ref = capi.block_solve(pm, K, links, B, damp, dm, gm)
        d_host = rel(delta[free], ref[free])
        d_own = rel(delta[free], np.linalg.solve(Hf + damp * np.diag(np.diag(Hf)), g[free] + gadd[free]))
        summary_line(f"solver rows, {name} (Bs {Bs}), damp {damp}: free entries vs host block solve of the masked system "
                     f"{d_host:.2e}, vs dense solve of the engine's free rows {d_own:.2e}")
        assert d_host < 1e-7 and d_own < 1e-7
    win.accept()
    moved = False
    for k in range(K):
        (p0, c0, s0), (p1, c1, s1) = start[k], win.get_keyframe(k)
        m = holds.get(k, 0)
        if m & POSE:
            assert np.array_equal(p0, p1), (name, k)
        if m & CODE:
            assert np.array_equal(c0, c1), (name, k)
        if m & SCALE:
            assert s0 == s1, (name, k)
        moved = moved or not (np.array_equal(p0, p1) and np.array_equal(c0, c1) and s0 == s1)
    assert moved
    win.close()


# ------------------------------------------------------------------------------------------------------ 3. dense edges
def test_holding_every_code_leaves_the_packed_buffer_alone_and_changes_the_step(capi):
    w, links, win, holds, _ = dense_case(capi, CODE)
    K, CS, B = len(w.keyframes), w.CS, 7 + w.CS
    plain = capi.Window(w)
    free = np.setdiff1d(np.arange(K * B), held_rows(holds, K, CS))
    for x in (win, plain):
        x.linearize()
    assert np.array_equal(win.packed_host(), plain.packed_host())
    for damp in (1e-3, 1e-1):
        win.solve(damp); plain.solve(damp)
        d = rel(win.delta()[free], plain.delta()[free])
        summary_line(f"solver rows, all codes held vs nothing held, damp {damp}: pose / scale step differs by {d:.2e}")
        assert d > 1e-3                                            # the code coupling is gone, not just hidden
    win.close(); plain.close()


# ------------------------------------------------------------------------------------------------------ 5. sharded
@pytest.mark.parametrize("rank", [0, 1])
def test_a_reduced_shard_takes_the_single_rank_step_bit_for_bit(capi, rank):
    """two shards on one device, keypoint links only, every code held: rank `rank` of two with the other rank's share from
    sage_window_emulate_peers sums to the single-rank system, so its compact solve is the single-rank window's"""
    w = make()
    holds = {k: CODE for k in range(len(w.keyframes))}
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    one, _ = all_keypoint_window(capi, w, holds=holds)
    st1 = capi.SageLmState(); st1.damp = 1e-3
    one.lm_step(st1, cfg)
    sh, _ = all_keypoint_window(capi, w, rank=rank, world=2, holds=holds)
    other, _ = all_keypoint_window(capi, w, rank=1 - rank, world=2, holds=holds)
    assert one.Bs == sh.Bs == other.Bs == 7
    other.linearize()
    rest = other.packed_tensor().clone().reshape(1, -1).contiguous()
    sh.set_allreduce(_NoPeers())
    sh.emulate_peers(rest)
    st2 = capi.SageLmState(); st2.damp = 1e-3
    sh.lm_step(st2, cfg)
    assert np.linalg.norm(one.delta()) > 0
    assert np.array_equal(sh.delta(), one.delta())
    assert st1.accepted == st2.accepted
    for k in range(len(w.keyframes)):
        for a, b in zip(one.get_keyframe(k), sh.get_keyframe(k)):
            assert np.array_equal(a, b)
    for win in (one, sh, other):
        win.close()


# ------------------------------------------------------------------------------------------------------ 6. recovery
def test_pose_scale_graph_recovers_on_the_compact_system(capi, orc):
    """twelve LM steps on the pose-scale graph, by the acceptance rule of test_pose_scale_graph_first_step_and_recovery: at
    most ten times the reference LM's distance (or 1e-6), the error down to 1e-6 of the first"""
    w, links, terms, holds = graph_scene()
    win = capi.Window(w, keypoint_links=links, keypoint_terms=terms, holds=holds, code_prior_weight=0.0)
    assert win.Bs == 7
    start = engine_vars(win)
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
    summary_line(f"solver rows, pose-scale graph recovery at Bs 7 (translation / scale / rotation): start {fmt(d0)}, engine "
                 f"{fmt(de)}, reference {fmt(dr)}; error {tr[0, 0]:.3f} -> {st.error:.2e} (reference {ref_first:.3f} -> "
                 f"{ref_err:.2e}), {int(tr[:, 2].sum())} of 12 accepted")
    for e, r in zip(de, dr):
        assert e <= max(10 * r, 1e-6), (de, dr)
    for k in range(len(w.keyframes)):                            # codes and keyframe 0: bit-equal to the start
        assert np.array_equal(final[k][2], start[k][2])
    assert np.array_equal(final[0][0], start[0][0]) and np.array_equal(final[0][1], start[0][1]) and final[0][3] == start[0][3]
    assert st.error <= 1e-6 * tr[0, 0]
    win.close()
