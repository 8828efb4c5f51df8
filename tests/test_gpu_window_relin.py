"""Partial relinearization of a window (sage_window_set_relinearization, SAGE_RELIN_STALE) against a twin window in
SAGE_RELIN_ALL at the same values -- the code path of every other test, not the code under test.

Every comparison is BYTE FOR BYTE (np.array_equal on the raw arrays): per-edge results are independent of each other -- own
partial records, one finalize workgroup, a fixed summation order -- so evaluating a subset computes the same bits.  Compared
per directed edge and factor type: sage_window_get_edge (AtA, Atb, error, inliers); and the whole packed buffer.

What a stale-mode linearize evaluates (SageEvalCounts) is predicted by `Model` below from sage_relin_plan and the rules of
include/sage_ba.h: the stale edges against the values of the last stale-mode linearize (every edge after a call that drops
them); their work items, ceil(sub-tiles / run length) per edge; the depth maps a stale edge reads whose code or scale bits
differ from what the map was last built from (unknown after an error pass at a candidate that is still on the device); the
gradients a stale geometric edge reads (its destination's) that were not built from the map as it stands."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import edge_scenes
from tests.test_gpu_psd_project import window_values
from tests.test_gpu_window_graph_terms import term_on_edge
from tests.test_gpu_window_loop_graph import lmg_term, mg_term, no_dense, rep_term

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, STATE = -1, -2, -4
POSE, CODE, SCALE = 1, 2, 4
GROUPS = ("pose", "code", "scale")
PHOTO_RUN, GEO_RUN = 1, 2          # the plan's run lengths at this size (window_plan.h: 120 sub-tiles in all), checked below


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


_windows = {}


def make(CS):
    if CS not in _windows:
        _windows[CS] = synth.make_window(K=4, H=64, W=80, FS=16, CS=CS, L=4, back_links=2, seed=3)
    return _windows[CS]


def ragged(w):
    """the same window with another number of samples per keyframe: a random location mask (tests/edge_scenes.py) over each
    keyframe's samples, cut to a length of its own -- 8, 5, 3 and 7 sub-tiles, the last ones partly filled"""
    kfs = []
    for k, (kf, n) in enumerate(zip(w.keyframes, (1901, 1153, 700, 1600))):
        keep = np.nonzero(edge_scenes.location_mask("random", w.H, w.W, seed=k).reshape(-1)[kf.loc1d] > 0)[0][:n]
        assert keep.size == n
        kfs.append(dataclasses.replace(kf, loc1d=kf.loc1d[keep].copy(), homo=kf.homo[keep].copy()))
    return dataclasses.replace(w, keyframes=kfs)


def moved(vals, k, group, amount=1.0):
    """the values with one group of keyframe k changed"""
    poses, codes, scales = (a.copy() for a in vals)
    if group == "pose":
        poses[k, 9:] += np.float32(0.002 * amount)
    elif group == "code":
        codes[k, 3] += np.float32(0.01 * amount)
    else:
        scales[k] *= np.float32(1.0 + 0.01 * amount)
    return poses, codes, scales


def everything_moved(vals):
    poses, codes, scales = (a.copy() for a in vals)
    poses[:, 9:] += np.float32(0.001)
    return poses, (codes * np.float32(1.03)).astype(np.float32), (scales * np.float32(1.01)).astype(np.float32)


def set_values(win, vals):
    for k in range(win.K):
        win.set_keyframe(k, vals[0][k], vals[1][k], float(vals[2][k]))


def get_values(win):
    v = [win.get_keyframe(k) for k in range(win.K)]
    return np.stack([x[0] for x in v]), np.stack([x[1] for x in v]), np.array([x[2] for x in v], np.float32)


def results(win):
    """every per-edge result and the packed buffer, as raw arrays"""
    out = {}
    for t in (0, 1):
        for e in range(2 * len(win.win.links)):
            r = win.get_edge(t, e)
            out[(t, e)] = (r["AtA"], r["Atb"], np.float32(r["error"]), np.float32(r["num_inliers"]))
    out["packed"] = win.packed_host().copy()
    return out


def assert_equal(got, want, what):
    assert got.keys() == want.keys()
    for key, w_ in want.items():
        g_ = got[key]
        if key == "packed":
            assert np.array_equal(g_, w_), (what, "packed", int((g_ != w_).sum()))
        else:
            for name, a, b in zip(("AtA", "Atb", "error", "inliers"), g_, w_):
                assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (what, key, name)


def compare_with_twin(win, twin, vals, what):
    """the twin, set to the same values, evaluates everything: the stale window's results are the same bytes"""
    set_values(twin, vals)
    twin.linearize()
    assert_equal(results(win), results(twin), what)


class Model:
    """what a stale-mode linearize has to evaluate (the module docstring)"""

    def __init__(self, capi, w, photo_run=PHOTO_RUN, geo_run=GEO_RUN, use_photo=True, use_geo=True):
        self.capi, self.w, self.K, self.CS = capi, w, len(w.keyframes), w.CS
        self.links = [(min(a, b), max(a, b)) for a, b in w.links]
        self.runs = {0: photo_run, 1: geo_run}
        self.use = {0: use_photo, 1: use_geo}
        self.snapshot = None
        self.maps = [None] * self.K            # (code bytes, scale bytes) the map was built from, or None
        self.grads = [False] * self.K

    def items(self, t, e):
        a, b = self.links[e // 2]
        tiles = -(-self.w.keyframes[a if e % 2 == 0 else b].loc1d.size // 256)
        return -(-tiles // self.runs[t])

    def all_counts(self):
        ne = 2 * len(self.links)
        return dict(photo_edges=ne * self.use[0], geo_edges=ne * self.use[1],
                    photo_items=sum(self.items(0, e) for e in range(ne)) * self.use[0],
                    geo_items=sum(self.items(1, e) for e in range(ne)) * self.use[1])

    def drop(self):
        self.snapshot = None

    def whole_depth_batch(self, vals):
        """an error pass: every map at these values (None: not known to the host), no gradient"""
        self.maps = [None if vals is None else (vals[1][k].tobytes(), vals[2][k].tobytes()) for k in range(self.K)]
        self.grads = [False] * self.K

    def linearize(self, vals, packed_current=True):
        ne = 2 * len(self.links)
        zero = dict(photo_edges=0, geo_edges=0, depth_maps=0, depth_grads=0, photo_items=0, geo_items=0)
        if self.snapshot is None:
            stale = {0: np.ones(ne, np.uint8), 1: np.ones(ne, np.uint8)}
        else:
            p = self.capi.relin_plan(self.K, self.CS, self.links, self.snapshot, vals)
            stale = {0: p["photo_stale"], 1: p["geo_stale"]}
        stale = {t: s * self.use[t] for t, s in stale.items()}
        self.snapshot = tuple(a.copy() for a in vals)
        n = dict(zero)
        n["photo_edges"], n["geo_edges"] = int(stale[0].sum()), int(stale[1].sum())
        n["photo_items"] = sum(self.items(0, e) for e in np.nonzero(stale[0])[0])
        n["geo_items"] = sum(self.items(1, e) for e in np.nonzero(stale[1])[0])
        need_map, need_grad = set(), set()
        for e in range(ne):
            a, b = self.links[e // 2]
            src, dst = (a, b) if e % 2 == 0 else (b, a)
            if stale[0][e] or stale[1][e]:
                need_map.add(src)
            if stale[1][e]:
                need_map.add(dst); need_grad.add(dst)
        for k in sorted(need_map):
            stamp = (vals[1][k].tobytes(), vals[2][k].tobytes())
            if self.maps[k] != stamp:
                self.maps[k], self.grads[k] = stamp, False
                n["depth_maps"] += 1
        for k in sorted(need_grad):
            if not self.grads[k]:
                self.grads[k] = True
                n["depth_grads"] += 1
        return n


def dense_counts(win):
    n = win.last_evaluation()
    n.pop("host_entries_pulled")
    return n


def stale_pair(capi, w, **kw):
    win, twin = capi.Window(w, **kw), capi.Window(w, **kw)
    win.set_relinearization(capi.SAGE_RELIN_STALE)
    return win, twin


def first_linearize(capi, win, twin, model, vals, what):
    """the first stale-mode linearize evaluates everything -- as the twin reports of its own"""
    win.linearize()
    n = dense_counts(win)
    assert n == model.linearize(vals), what
    compare_with_twin(win, twin, vals, what)
    t = dense_counts(twin)
    assert {k: t[k] for k in model.all_counts()} == model.all_counts(), (what, "the run lengths this module assumes")
    assert {k: n[k] for k in model.all_counts()} == model.all_counts(), what
    return n


# ----------------------------------------------------------------------------------- 1. one group of one keyframe at a time
@pytest.mark.parametrize("CS", [16, 32])
def test_one_group_of_one_keyframe_at_a_time(capi, CS):
    w = make(CS)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    vals = window_values(w)
    first = first_linearize(capi, win, twin, model, vals, "first")
    assert first["depth_maps"] == first["depth_grads"] == 4
    step = 0
    for k in range(4):
        for group in GROUPS:
            step += 1
            vals = moved(vals, k, group, amount=step)
            set_values(win, vals)
            win.linearize()
            n = dense_counts(win)
            assert n == model.linearize(vals), (k, group, n)
            assert 0 < n["geo_edges"] < 10 and n["photo_edges"] <= n["geo_edges"]
            assert (n["depth_maps"], n["depth_grads"]) == ((0, 0) if group == "pose" else (1, 1)), (k, group)
            compare_with_twin(win, twin, vals, (k, group))
    win.close(); twin.close()


# ------------------------------------------------------------- 2. an error pass at other values in between: the two traps
@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("how", ["candidate", "prepass"])
def test_error_pass_at_other_values_in_between(capi, CS, how):
    """the linearization's {error, inliers} of the clean edges survive the pass, and every depth map a stale edge reads is
    rebuilt: the pass has overwritten all of them"""
    w = make(CS)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "first")
    before = results(win)
    for i, (k, group) in enumerate(((3, "code"), (0, "pose"), (1, "scale"))):
        if how == "candidate":
            win.solve(1e-2, want_norm=False)
            win.error(1)                                                 # at the candidate, whose host mirror is on its way
            model.whole_depth_batch(None)
        else:
            other = everything_moved(vals)
            assert win.prepass(*other, jacobians=False)                  # error only, at other values: they become current
            model.whole_depth_batch(other)
        vals = moved(vals, k, group, amount=i + 1)
        if how == "candidate":
            set_values(win, vals)
            win.linearize()
        else:
            assert win.prepass(*vals, jacobians=True)
        n = dense_counts(win)
        assert n == model.linearize(vals), (how, k, group, n)
        assert n["geo_edges"] < 10 and n["depth_maps"] >= 3              # the keyframe and its neighbours, not one map
        now = results(win)
        clean = [key for key in before if key != "packed" and all(np.array_equal(a, b) for a, b in zip(before[key], now[key]))]
        assert len(clean) >= 20 - n["geo_edges"] - n["photo_edges"]      # (the clean edges kept every byte, statistics included)
        compare_with_twin(win, twin, vals, (how, k, group))
        before = now
    win.close(); twin.close()


# ------------------------------------------------------------------------------- 3. run lengths: records != work items, ragged
@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("runs", [8, 3, 5])
def test_forced_run_lengths(capi, CS, runs):
    """8: the record cadence of 4 gives 3 records and 2 work items per 12-sub-tile edge; 5: a ragged last run on every
    edge (5 + 5 + 2); 3: four full runs at this size (3 072 samples per keyframe are exactly 12 sub-tiles; runs of 3 meet
    ragged edges in test_edges_of_different_lengths).  A new run length drops every per-edge result"""
    w = make(CS)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "plan's runs")
    win.set_runs(runs); twin.set_runs(runs)
    model.runs[0] = runs
    model.drop()
    first_linearize(capi, win, twin, model, vals, f"runs of {runs}")
    for k, group in ((2, "code"), (3, "pose"), (0, "scale")):
        vals = moved(vals, k, group)
        set_values(win, vals)
        win.linearize()
        n = dense_counts(win)
        assert n == model.linearize(vals), (runs, k, group, n)
        assert n["photo_items"] == n["photo_edges"] * -(-12 // runs)
        compare_with_twin(win, twin, vals, (runs, k, group))
    win.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 4. edges of different lengths
@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("runs", [0, 3])
def test_edges_of_different_lengths(capi, CS, runs):
    w = ragged(make(CS))
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    assert sorted({model.items(0, e) for e in range(10)}) == [3, 5, 7, 8]
    vals = window_values(w)
    if runs:
        win.set_runs(runs); twin.set_runs(runs)
        model.runs[0] = runs
    first_linearize(capi, win, twin, model, vals, "ragged")
    for k, group in ((1, "code"), (2, "pose"), (3, "scale"), (0, "code")):
        vals = moved(vals, k, group)
        set_values(win, vals)
        win.linearize()
        n = dense_counts(win)
        assert n == model.linearize(vals), (k, group, n)
        compare_with_twin(win, twin, vals, (k, group))
    win.close(); twin.close()


# ------------------------------------------------------------------------------------------------------- 5. next to the terms
def terms_of(w, links):
    rng = np.random.default_rng(7)
    ne = 2 * len(links)
    kp = [rep_term(w, links, 0), mg_term(w, links, 3), lmg_term(w, links, ne - 1), rep_term(w, links, ne - 2)]
    graph = [dict(kind="scale_prior", kf=2, target_scale0=float(np.float32(w.keyframes[2].scale * 1.1)), weight=50.0),
             term_on_edge(w, links, 1, "rel_pose", rng), term_on_edge(w, links, ne - 1, "rel_pose_scale", rng)]
    return kp, graph


def term_systems(win):
    out = [win.get_keypoint_term(i) for i in range(win.num_keypoint_terms())]
    return out + [win.get_graph_term(i) for i in range(win.num_graph_terms())]


def assert_terms_equal(win, twin, what):
    for i, (a, b) in enumerate(zip(term_systems(win), term_systems(twin))):
        assert np.array_equal(a["AtA"], b["AtA"]) and np.array_equal(a["Atb"], b["Atb"]) and a["error"] == b["error"], (what, i)


@pytest.mark.parametrize("CS", [16, 32])
def test_keypoint_and_graph_terms_next_to_the_dense_edges(capi, CS):
    """the terms are evaluated in full whatever is stale; their share of the packed buffer and of its tail is the twin's"""
    w = make(CS)
    kp, graph = terms_of(w, w.links)
    win, twin = stale_pair(capi, w, keypoint_terms=kp, graph_terms=graph)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "with terms")
    for k, group in ((3, "pose"), (2, "scale"), (0, "code")):
        vals = moved(vals, k, group)
        set_values(win, vals)
        win.linearize()
        assert dense_counts(win) == model.linearize(vals), (k, group)
        compare_with_twin(win, twin, vals, (k, group))
        assert_terms_equal(win, twin, (k, group))
    win.close(); twin.close()


def test_keypoint_links_only(capi):
    """no dense edge at all: stale mode launches no dense kernel and still evaluates the terms and assembles"""
    w = make(32)
    kp, graph = terms_of(w, w.links)
    bare = no_dense(w)
    win = capi.Window(bare, keypoint_links=w.links, keypoint_terms=kp, graph_terms=graph)
    twin = capi.Window(bare, keypoint_links=w.links, keypoint_terms=kp, graph_terms=graph)
    win.set_relinearization(capi.SAGE_RELIN_STALE)
    zero = dict(photo_edges=0, geo_edges=0, depth_maps=0, depth_grads=0, photo_items=0, geo_items=0)
    vals = window_values(w)
    for step, (k, group) in enumerate(((None, None), (1, "pose"), (3, "scale"))):
        if k is not None:
            vals = moved(vals, k, group)
            set_values(win, vals)
        win.linearize()
        assert dense_counts(win) == zero
        set_values(twin, vals)
        twin.linearize()
        assert np.array_equal(win.packed_host(), twin.packed_host()), step
        assert_terms_equal(win, twin, step)
        assert np.abs(win.packed_host()).max() > 0
    win.close(); twin.close()


# ------------------------------------------------------------------------------------------- 6. nothing stale, everything stale
@pytest.mark.parametrize("CS", [16, 32])
def test_nothing_stale_and_everything_stale(capi, CS):
    w = make(CS)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "first")
    before = results(win)
    zero = dict(photo_edges=0, geo_edges=0, depth_maps=0, depth_grads=0, photo_items=0, geo_items=0)
    win.linearize()                                                       # the same values, the packed system current
    assert dense_counts(win) == zero == model.linearize(vals)
    assert_equal(results(win), before, "nothing stale")
    set_values(win, vals)                                                 # the same bits written again: still nothing
    win.linearize()
    assert dense_counts(win) == zero
    assert_equal(results(win), before, "the same values set again")
    vals = everything_moved(vals)
    set_values(win, vals)
    win.linearize()
    n = dense_counts(win)
    assert n == model.linearize(vals) and {k: n[k] for k in model.all_counts()} == model.all_counts()
    assert (n["depth_maps"], n["depth_grads"]) == (4, 4)
    compare_with_twin(win, twin, vals, "everything stale")
    # a switch of the mode marks every edge stale; SAGE_RELIN_ALL evaluates everything whatever the values
    win.set_relinearization(capi.SAGE_RELIN_ALL)
    win.linearize()
    assert {k: dense_counts(win)[k] for k in model.all_counts()} == model.all_counts()
    win.set_relinearization(capi.SAGE_RELIN_STALE)
    win.linearize()
    n = dense_counts(win)
    assert {k: n[k] for k in model.all_counts()} == model.all_counts() and (n["depth_maps"], n["depth_grads"]) == (4, 4)
    assert_equal(results(win), results(twin), "after the switches")
    win.reset()                                                           # ... and so does a reset
    vals = window_values(w)
    win.linearize()
    assert {k: dense_counts(win)[k] for k in model.all_counts()} == model.all_counts()
    compare_with_twin(win, twin, vals, "after a reset")
    win.close(); twin.close()


# --------------------------------------------------------------------------------------------------------- 7. after an LM step
def test_lm_step_leaves_every_edge_stale(capi):
    """the step's merged linearize leaves mixed per-edge results: the next stale-mode linearize evaluates every edge"""
    w = make(32)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "first")
    st = capi.SageLmState(); cfg = capi.lm_config_default(); cfg.max_inner_evals = 1
    win.lm_step(st, cfg)
    assert st.accepted == 1
    vals = get_values(win)
    win.linearize()
    n = dense_counts(win)
    assert {k: n[k] for k in model.all_counts()} == model.all_counts()
    compare_with_twin(win, twin, vals, "after an LM step")
    # ... and so after a step that follows a stale-mode linearize
    win.lm_step(st, cfg)
    win.linearize()
    n = dense_counts(win)
    assert {k: n[k] for k in model.all_counts()} == model.all_counts()
    compare_with_twin(win, twin, get_values(win), "after a second LM step")
    win.close(); twin.close()


# ----------------------------------------------------------------------------------------------- 8. the solve behind the system
@pytest.mark.parametrize("holds", [{0: POSE | CODE | SCALE, 2: CODE}, {k: CODE for k in range(4)}], ids=["held-group", "rows-dropped"])
def test_solve_after_a_stale_linearize(capi, holds):
    w = make(16)
    win, twin = stale_pair(capi, w, holds=holds)
    assert (win.Bs < win.B) == (len(holds) == 4)
    model = Model(capi, w)
    vals = window_values(w)
    first_linearize(capi, win, twin, model, vals, "first")
    for k, group in ((3, "pose"), (1, "scale")):
        vals = moved(vals, k, group)
        set_values(win, vals)
        win.linearize()
        assert dense_counts(win) == model.linearize(vals)
        compare_with_twin(win, twin, vals, (k, group))
        sn = win.solve(1e-3)
        assert sn == twin.solve(1e-3) and sn > 0
        assert np.array_equal(win.delta(), twin.delta())
        for kf in range(4):
            for a, b in zip(win.get_keyframe(kf), twin.get_keyframe(kf)):
                assert np.array_equal(a, b)
    win.close(); twin.close()


# ------------------------------------------------------------------------------------ 9. the ISAM2 pattern through the cache
def served(win, modes=(0, 1)):
    out = {}
    for t in (0, 1):
        for e in range(2 * len(win.win.links)):
            for mode in modes:
                out[(t, e, mode)] = win.factor(t, e, psd_mode=mode)
            out[(t, e, "error")] = win.factor_error(t, e)
    return out


def assert_served_equal(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        if key[2] == "error":
            assert a[key] == b[key], (what, key)
            continue
        (ba, ga, fa, da), (bb, gb, fb, db) = a[key], b[key]
        assert da == db and fa == fb, (what, key)
        assert all(np.array_equal(ba[k], bb[k]) for k in bb) and all(np.array_equal(x, y) for x, y in zip(ga, gb)), (what, key)


@pytest.mark.parametrize("CS", [16, 32])
def test_isam2_pattern_through_the_factor_cache(capi, CS):
    """prepass(theta, jacobians) -> prepass(x, error only) -> prepass(theta', jacobians), theta' = theta except pose and code
    of one keyframe: only the stale edges are evaluated and only their rows cross to the host"""
    w = make(CS)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    theta = window_values(w)
    assert win.prepass(*theta, jacobians=True)
    n = win.last_evaluation()
    assert n.pop("host_entries_pulled") == 20 and n == model.linearize(theta)
    assert twin.prepass(*theta, jacobians=True) and twin.last_evaluation()["host_entries_pulled"] == 20
    assert_served_equal(served(win), served(twin), "theta")
    for k in (3, 1):
        x = everything_moved(theta)
        assert win.prepass(*x, jacobians=False)
        model.whole_depth_batch(x)
        errs = [win.factor_error(t, e) for t in (0, 1) for e in range(10)]
        assert twin.prepass(*x, jacobians=False)
        assert errs == [twin.factor_error(t, e) for t in (0, 1) for e in range(10)]
        assert win._cached_factor("sage_window_factor", (0, 0), 1, False)[0] == STATE     # (the cache's key is x now)
        theta = moved(moved(theta, k, "pose"), k, "code")
        assert win.prepass(*theta, jacobians=True)
        n = win.last_evaluation()
        pulled = n.pop("host_entries_pulled")
        want = model.linearize(theta)
        assert n == want and pulled == want["photo_edges"] + want["geo_edges"] < 20, (k, n, pulled)
        assert twin.prepass(*theta, jacobians=True)
        assert_served_equal(served(win), served(twin), ("theta'", k))
        assert_equal(results(win), results(twin), ("theta'", k))
        assert not win.prepass(*theta, jacobians=True)                    # the cache holds theta'
    win.prepare_factors(1, 2); twin.prepare_factors(1, 2)                 # afterwards every factor is still served
    assert_served_equal(served(win, (1,)), served(twin, (1,)), "prepared")
    win.close(); twin.close()


# --------------------------------------------------------------------------------------------------------- 10. the fluid loop
def test_fluid_loop_with_explicit_marks(capi):
    """linearize (stale) -> solve -> marks -> masked accept, four times; the twin takes the same calls in SAGE_RELIN_ALL"""
    w = make(16)
    win, twin = stale_pair(capi, w)
    model = Model(capi, w)
    newest = np.array([0, 0, 0, POSE | CODE], np.int32)
    plan = [newest, np.zeros(4, np.int32), newest, np.array([0, SCALE, 0, 0], np.int32)]
    evaluated = []
    vals = window_values(w)
    for it, marks in enumerate(plan):
        win.linearize(); twin.linearize()
        n = dense_counts(win)
        assert n == model.linearize(vals), (it, n)
        evaluated.append(n["photo_edges"] + n["geo_edges"])
        assert np.array_equal(win.packed_host(), twin.packed_host()), it
        assert win.solve(1e-2) == twin.solve(1e-2)
        assert np.array_equal(win.delta(), twin.delta()), it
        win.accept_marked(marks); twin.accept_marked(marks)
        new = get_values(win)
        for a, b in zip(new, get_values(twin)):
            assert np.array_equal(a, b), it
        for k in range(4):                                                 # only the marked groups moved
            for g, (bit, a, b) in enumerate(zip((POSE, CODE, SCALE), vals, new)):
                assert (a[k].tobytes() != b[k].tobytes()) == bool(marks[k] & bit), (it, k, g)
        vals = new
    assert evaluated[0] == 20 and evaluated[2] == 0 and 0 < evaluated[1] < 20 and 0 < evaluated[3] < 20
    # the window's own marks: the groups of the last delta over the mapper's thresholds, as the stateless call finds them
    win.linearize(); twin.linearize()
    win.solve(1e-2)
    t = capi.relin_thresholds()
    marks, n_marked = win.relin_marks(t)
    ref, n_ref = capi.relin_marks(win.delta(), 4, 16, t)
    assert np.array_equal(marks, ref) and n_marked == n_ref > 0
    compare_with_twin(win, twin, vals, "after the loop")
    win.close(); twin.close()


def test_marks_leave_held_groups_alone(capi):
    w = make(16)
    win = capi.Window(w, holds={0: POSE | CODE | SCALE, 2: CODE})
    win.linearize()
    win.solve(1e-2)
    t = capi.relin_thresholds(pose=0.0, code=0.0, scale=0.0)               # everything that moves at all is marked
    marks, n = win.relin_marks(t)
    assert marks[0] == 0 and marks[2] & CODE == 0 and marks[1] == marks[3] == POSE | CODE | SCALE
    before = get_values(win)
    win.accept_marked(np.full(4, POSE | CODE | SCALE, np.int32))           # marking a held group moves nothing of it
    after = get_values(win)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(before, after)) and np.array_equal(before[1][2], after[1][2])
    assert not np.array_equal(before[0][1], after[0][1]) and not np.array_equal(before[1][3], after[1][3])
    bad = np.array([0, 8, 0, 0], np.int32)
    assert capi.lib().sage_window_accept_marked(win.h, bad.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    win.close()


# ------------------------------------------------------------------------------------------------------ 11. what is refused
def test_status_codes_on_a_device(capi):
    L = capi.lib()
    w = make(16)
    sharded = capi.Window(w, rank=0, world=2)
    assert sharded.set_relinearization(capi.SAGE_RELIN_STALE, check=False) == UNSUPPORTED
    assert sharded.set_relinearization(capi.SAGE_RELIN_ALL, check=False) == 0
    sharded.close()
    win = capi.Window(w)
    for mode in (2, -1):
        assert win.set_relinearization(mode, check=False) == INVALID
    assert L.sage_window_last_evaluation(win.h, None) == INVALID
    assert L.sage_window_relin_marks(win.h, None, None, None) == INVALID
    assert L.sage_window_accept_marked(win.h, None) == INVALID
    h2 = C.c_void_p()                                                      # a window that was never finalized
    assert L.sage_window_create(C.byref(win.cfg), C.c_void_p(0), C.byref(h2)) == 0
    n = capi.SageEvalCounts(); t = capi.relin_thresholds(); m = np.zeros(4, np.int32)
    mp = m.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.sage_window_set_relinearization(h2, capi.SAGE_RELIN_STALE) == STATE
    assert L.sage_window_set_relinearization(h2, 5) == INVALID
    assert L.sage_window_last_evaluation(h2, C.byref(n)) == STATE
    assert L.sage_window_relin_marks(h2, C.byref(t), mp, None) == STATE
    assert L.sage_window_accept_marked(h2, mp) == STATE
    L.sage_window_destroy(h2)
    win.close()
