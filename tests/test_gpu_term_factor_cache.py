"""A window's keypoint and graph terms served from the gtsam factor cache (sage_window_prepass, sage_window_keypoint_factor /
sage_window_graph_factor and their _error calls, both eager projections) against the host definition
sage_term_factor_blocks on the same linearisation (sage_window_get_keypoint_term / sage_window_get_graph_term).

Bars.  Lazy reads and the host-thread preparation: bit for bit.  The device preparation: bar 1 of
tests/test_gpu_psd_project.py with the kind's own dimension, ||blocks - host||_F <= 32 D_own 2^-52 ||B||_F over all blocks
of the factor, B the symmetrised own-dimension matrix; g and f byte for byte.  Errors of an error-only prepass against a
linearising one, and their sum against the window's total: TOL_TOTAL of tests/test_gpu_window_keypoints.py.  One test reads
the dense factors and every term group of one window through the cache they share, at the same bars."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import psd_ref
from tests.test_gpu_psd_project import stats_bytes, window_values
from tests.test_gpu_window_graph_terms import term_on_edge
from tests.test_gpu_window_keypoints import LOSSES, TOL_TOTAL, mg_term, rep_term
from tests.test_gpu_window_loop_graph import lmg_term

pytestmark = pytest.mark.gpu

EPS = psd_ref.EPS
INVALID, STATE = -1, -4
KP, GRAPH = 0, 1


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
        _windows[CS] = synth.make_window(K=6, H=48, W=64, FS=16, CS=CS, L=3, n_samples=900, seed=5)
    return _windows[CS]


def keypoint_terms(w):
    """every group: reprojection N = 1 / 96 and two on one edge; match geometry with every loss (N = 64) and N = 1;
    loop-MG N = 64 and N = 1"""
    ne = 2 * len(w.links)
    kp = [rep_term(w, 0, n=1), rep_term(w, 1, n=96), rep_term(w, 1, n=96, seed=1)]
    kp += [mg_term(w, (2 + i) % ne, loss, n=64) for i, loss in enumerate(LOSSES)]
    kp += [mg_term(w, 3, "fair", n=1, seed=2), lmg_term(w, w.links, 4 % ne, n=64), lmg_term(w, w.links, 5 % ne, n=1, seed=1)]
    return kp


def graph_terms(w):
    rng = np.random.default_rng(11)
    ne = 2 * len(w.links)
    return [dict(kind="scale_prior", kf=2, target_scale0=float(np.float32(w.keyframes[2].scale * 1.1)), weight=50.0),
            term_on_edge(w, w.links, ne - 1, "rel_pose", rng), term_on_edge(w, w.links, ne - 2, "rel_pose_scale", rng),
            term_on_edge(w, w.links, ne - 2, "rel_pose", rng)]


def group2_terms(w):
    """only the D = 14 group: loop-MG and the three graph kinds"""
    return [lmg_term(w, w.links, 0, n=64), lmg_term(w, w.links, 1, n=1, seed=1)], graph_terms(w)


def moved_values(w, seed=0):
    """values that differ from the ones the keyframes were added with"""
    poses, codes, scales = window_values(w)
    r = np.random.default_rng([17, seed])
    poses = poses.copy(); poses[:, 9:] += r.normal(0.0, 0.002, poses[:, 9:].shape).astype(np.float32)
    codes = (codes * np.float32(1.03)).astype(np.float32)
    scales = (scales * np.float32(1.01)).astype(np.float32)
    return poses, codes, scales


def family_kind(capi, win, fam, i):
    if fam == KP:
        return capi.KP_KINDS.get(win.keypoint_terms[i]["kind"], win.keypoint_terms[i]["kind"])
    return capi.GRAPH_KINDS.get(win.graph_terms[i]["kind"], win.graph_terms[i]["kind"])


def all_ids(win):
    return [(KP, i) for i in range(len(win.keypoint_terms))] + [(GRAPH, i) for i in range(len(win.graph_terms))]


def systems_now(win, ids=None):
    """the device's term systems as they stand: right after a prepass, what the cache holds"""
    return {(fam, i): (win.get_keypoint_term(i) if fam == KP else win.get_graph_term(i)) for fam, i in (ids or all_ids(win))}


def serve(win, fam, i, mode, check=True):
    return win.keypoint_factor(i, mode, check=check) if fam == KP else win.graph_factor(i, mode, check=check)


def serve_error(win, fam, i, check=True):
    return win.keypoint_factor_error(i, check=check) if fam == KP else win.graph_factor_error(i, check=check)


DIMS = {(KP, 0): lambda CS: [6, 6, CS, 1], (KP, 1): lambda CS: [6, 6, CS, CS, 1, 1], (KP, 2): lambda CS: [6, 6, 1, 1],
        (GRAPH, 0): lambda CS: [6, 6, 1, 1], (GRAPH, 1): lambda CS: [6, 6], (GRAPH, 2): lambda CS: [1]}


def own_matrix(fam, kind, CS, A):
    Do = sum(DIMS[(fam, kind)](CS))
    first = 12 if (fam, kind) == (GRAPH, 2) else 0
    return A[first:first + Do, first:first + Do].astype(np.float64)


def assert_serves_exactly(capi, win, CS, systems, modes):
    for (fam, i), h in systems.items():
        kind = family_kind(capi, win, fam, i)
        for mode in modes:
            blocks, gs, f, dims = serve(win, fam, i, mode)
            rb, rg, rdims = capi.term_factor_blocks(fam, kind, CS, h["AtA"], h["Atb"], mode)
            assert dims == rdims == DIMS[(fam, kind)](CS), (fam, i)
            assert sorted(blocks) == sorted(rb)
            assert all(blocks[k].tobytes() == rb[k].tobytes() for k in rb), (fam, i, mode)
            assert len(gs) == len(rg) and all(a.tobytes() == b.tobytes() for a, b in zip(gs, rg)), (fam, i, mode)
            assert f == float(h["error"]), (fam, i)


def assert_serves_within_the_bar(capi, win, CS, systems, label):
    worst = 0.0
    for (fam, i), h in systems.items():
        kind = family_kind(capi, win, fam, i)
        blocks, gs, f, dims = serve(win, fam, i, 1)
        rb, rg, rdims = capi.term_factor_blocks(fam, kind, CS, h["AtA"], h["Atb"], 1)
        assert dims == rdims
        B = psd_ref.symmetrised(own_matrix(fam, kind, CS, h["AtA"]))
        bar = 32 * sum(dims) * EPS * np.linalg.norm(B)
        err = np.sqrt(sum(np.sum((blocks[k] - rb[k]) ** 2) for k in rb))
        worst = max(worst, err / bar if bar > 0 else float(err > 0))
        print("%s: term (%d, %d) kind %d D_own %d: ||blocks - host||_F %.3g, bar %.3g" % (label, fam, i, kind, sum(dims), err, bar))
        assert err <= bar, (fam, i, err, bar)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gs, rg)), (fam, i)
        assert f == float(h["error"]), (fam, i)
    return worst


def dense_factors(win, ne, mode):
    out = {}
    for t in (0, 1):
        for e in range(ne):
            blocks, gs, f, dims = win.factor(t, e, psd_mode=mode)
            out[(t, e)] = b"".join(blocks[k].tobytes() for k in sorted(blocks)) + b"".join(g.tobytes() for g in gs) + np.float64(f).tobytes()
    return out


# ------------------------------------------------------------------------------------------- 1, 2. lazy and host-prepared
@pytest.mark.parametrize("CS", [16, 32])
def test_every_term_is_served_bit_for_bit_lazily_and_after_the_host_preparation(capi, CS):
    w = make(CS)
    win = capi.Window(w, keypoint_terms=keypoint_terms(w), graph_terms=graph_terms(w))
    assert win.prepass(*moved_values(w), jacobians=True)
    systems = systems_now(win)
    # the small terms are the ones whose projection does work: fp32 rounding leaves a rank-deficient AtA indefinite
    assert any(np.linalg.eigvalsh(psd_ref.symmetrised(h["AtA"])).min() < 0 for h in systems.values())
    assert all(h["AtA"].any() for h in systems.values())
    assert_serves_exactly(capi, win, CS, systems, (0, 1, 2))                 # lazy
    for mode in (1, 2):
        win.prepare_factors(mode, 3)
        assert_serves_exactly(capi, win, CS, systems, (mode,))               # cut from the prepared matrix
        assert_serves_exactly(capi, win, CS, systems, (0,))                  # another mode: lazy again
    for fam, i in all_ids(win):
        assert serve_error(win, fam, i) == float(systems[(fam, i)]["error"])
    assert not win.prepass(*moved_values(w), jacobians=True)                 # the same values: a cache hit
    win.close()


# ------------------------------------------------------------------------------------------- 3, 4. the device preparation
@pytest.mark.parametrize("CS", [16, 32])
def test_the_device_preparation_covers_the_terms_and_leaves_the_dense_factors_alone(capi, CS):
    w = make(CS)
    ne = 2 * len(w.links)
    win, twin = capi.Window(w, keypoint_terms=keypoint_terms(w), graph_terms=graph_terms(w)), capi.Window(w)
    values = moved_values(w)
    assert win.prepass(*values, jacobians=True) and twin.prepass(*values, jacobians=True)
    systems = systems_now(win)
    worst = win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 5                        # two dense types + three term groups
    assert worst.status == 0 and 0 < worst.sweeps < 30
    assert_serves_within_the_bar(capi, win, CS, systems, "CS %d" % CS)
    twin.prepare_factors_device()
    assert twin.prepare_factors_device_launches() == 2
    assert dense_factors(win, ne, 1) == dense_factors(twin, ne, 1)           # no change for what exists
    first = {k: serve(win, *k, 1)[0] for k in systems}
    again = win.prepare_factors_device()                                     # prepared already
    assert win.prepare_factors_device_launches() == 0 and stats_bytes(again) == stats_bytes(worst)
    # a host call with another mode replaces the preparation; the device call brings the same bytes back
    win.prepare_factors(2, 0)
    assert_serves_exactly(capi, win, CS, systems, (2,))
    win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 5
    for k in systems:
        b = serve(win, *k, 1)[0]
        assert all(b[j].tobytes() == first[k][j].tobytes() for j in b)
    # a recomputing prepass drops the preparation: the lazy host path, bit for bit, at the new values
    values2 = moved_values(w, seed=1)
    assert win.prepass(*values2, jacobians=True)
    systems2 = systems_now(win)
    assert sum(not np.array_equal(systems2[k]["AtA"], systems[k]["AtA"]) for k in systems) >= len(systems) // 2
    assert_serves_exactly(capi, win, CS, systems2, (1,))
    win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 5
    assert_serves_within_the_bar(capi, win, CS, systems2, "CS %d, second values" % CS)
    win.close(); twin.close()


def test_the_device_preparation_uploads_the_cache_when_the_terms_have_moved_on(capi):
    CS = 16
    w = make(CS)
    kp, gt = group2_terms(w)
    win = capi.Window(w, keypoint_terms=kp, graph_terms=gt)                  # only group 2 has entries
    assert win.prepass(*moved_values(w), jacobians=True)
    systems_x = systems_now(win)
    pose1, code1, s1 = win.get_keyframe(1)
    pose1 = pose1.copy(); pose1[9:] += np.float32(0.004)
    win.set_keyframe(1, pose1, code1 * np.float32(1.05), s1 * np.float32(1.02))
    win.linearize()                                                          # the device's term systems are no longer X's
    systems_y = systems_now(win)
    assert sum(not np.array_equal(systems_y[k]["AtA"], systems_x[k]["AtA"]) for k in systems_x) >= 2
    worst = win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 3 and worst.status == 0
    assert_serves_within_the_bar(capi, win, CS, systems_x, "upload path")
    # REL_POSE is exactly singular (its pose1 block is minus its pose0 block) and sits in a zero-padded 14 x 14
    rp = [i for i, t in enumerate(gt) if t["kind"] == "rel_pose"]
    for i in rp:
        A = systems_x[(GRAPH, i)]["AtA"]
        assert not A[12:].any() and not A[:, 12:].any() and A[:12, :12].any()
    win.close()


# ------------------------------------------------------------------------------------------- one cache for both
def read_all(win, ne, mode):
    """every dense factor and every term of the window from the cache -> {key: (blocks, gs, f, dims)}"""
    out = {("dense", t, e): win.factor(t, e, psd_mode=mode) for t in (0, 1) for e in range(ne)}
    out.update({(fam, i): serve(win, fam, i, mode) for fam, i in all_ids(win)})
    return out


def same_bytes(a, b):
    return (a[3] == b[3] and a[2] == b[2] and sorted(a[0]) == sorted(b[0]) and all(a[0][k].tobytes() == b[0][k].tobytes() for k in b[0])
            and len(a[1]) == len(b[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])))


def test_dense_factors_and_every_term_group_go_through_one_cache(capi):
    """the smallest window that fills all five slots (both dense types, one term of every kind, N = 1): (a) the host-thread
    preparation serves what the lazy read serves, byte for byte, in every mode and for every factor; (b) after another
    linearize the device preparation uploads every slot's cached systems, launches once per slot and serves mode 1 within
    this file's device bar of (a)'s lazy host read, g and f byte for byte"""
    CS = 16
    w = synth.make_window(K=3, H=48, W=64, FS=16, CS=CS, L=3, n_samples=300, seed=5)
    ne = 2 * len(w.links)
    rng = np.random.default_rng(13)
    kp = [rep_term(w, 0, n=1), mg_term(w, 1 % ne, "fair", n=1), lmg_term(w, w.links, 2 % ne, n=1)]
    gt = [dict(kind="scale_prior", kf=1, target_scale0=float(np.float32(w.keyframes[1].scale * 1.1)), weight=50.0),
          term_on_edge(w, w.links, ne - 1, "rel_pose", rng), term_on_edge(w, w.links, 0, "rel_pose_scale", rng)]
    win = capi.Window(w, keypoint_terms=kp, graph_terms=gt)
    assert win.prepass(*moved_values(w), jacobians=True)
    own = {("dense", t, e): win.get_edge(t, e)["AtA"].astype(np.float64) for t in (0, 1) for e in range(ne)}
    own.update({(fam, i): own_matrix(fam, family_kind(capi, win, fam, i), CS, h["AtA"]) for (fam, i), h in systems_now(win).items()})
    # (a)
    lazy = {mode: read_all(win, ne, mode) for mode in (0, 1, 2)}
    assert set(lazy[1]) == set(own) and len(own) == 2 * ne + 6
    assert any(not same_bytes(lazy[0][k], lazy[1][k]) for k in own if k[0] == "dense")      # the projections do work
    assert any(not same_bytes(lazy[0][k], lazy[1][k]) for k in own if k[0] != "dense")
    for prepared in (1, 2, 0):
        win.prepare_factors(prepared, 2)
        for mode in (prepared, 0, 1, 2):
            again = read_all(win, ne, mode)
            assert all(same_bytes(again[k], lazy[mode][k]) for k in own), (prepared, mode)
    # (b)
    win.linearize()
    worst = win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 5 and worst.status == 0
    got = read_all(win, ne, 1)
    for k, ref in lazy[1].items():
        blocks, gs, f, dims = got[k]
        assert dims == ref[3]
        bar = 32 * sum(dims) * EPS * np.linalg.norm(psd_ref.symmetrised(own[k]))
        err = np.sqrt(sum(np.sum((blocks[j] - ref[0][j]) ** 2) for j in ref[0]))
        print("%s D_own %d: ||blocks - host||_F %.3g, bar %.3g" % (k, sum(dims), err, bar))
        assert err <= bar, (k, err, bar)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gs, ref[1])) and f == ref[2], k
    win.close()


# ------------------------------------------------------------------------------------------- 5. the error-only prepass
def test_an_error_only_prepass_serves_every_error_and_no_factor(capi):
    CS = 32
    w = make(CS)
    ne = 2 * len(w.links)
    kw = dict(keypoint_terms=keypoint_terms(w), graph_terms=graph_terms(w), code_prior_weight=0.0, scale_prior_weight=0.0,
              pose_prior_weight=0.0)                                         # (no priors: the total is the factors' sum)
    win, lin = capi.Window(w, **kw), capi.Window(w, **kw)
    values = moved_values(w)
    assert win.prepass(*values, jacobians=False) and lin.prepass(*values, jacobians=True)
    total = 0.0
    for fam, i in all_ids(win):
        e, ref = serve_error(win, fam, i), serve_error(lin, fam, i)
        assert ref > 0 and e == pytest.approx(ref, rel=TOL_TOTAL), (fam, i)
        total += e
        assert serve(win, fam, i, 1, check=False)[0] == STATE
    total += sum(win.factor_error(t, e) for t in (0, 1) for e in range(ne))
    assert total == pytest.approx(win.total_error(False), rel=TOL_TOTAL)
    with pytest.raises(capi.SageError) as ei:
        win.prepare_factors_device()
    assert ei.value.code == STATE
    assert win.prepass(*values, jacobians=True)                              # the linearisation on top: factors are served
    assert serve(win, KP, 0, 1, check=False)[0] == 0
    win.close(); lin.close()


# ------------------------------------------------------------------------------------------- 6. shards
def test_two_shards_on_one_device_serve_their_own_terms(capi):
    CS = 32
    w = make(CS)
    kp, gt = keypoint_terms(w), graph_terms(w)
    one = capi.Window(w, keypoint_terms=kp, graph_terms=gt)
    shards = [capi.Window(w, rank=r, world=2, keypoint_terms=kp, graph_terms=gt) for r in range(2)]
    values = moved_values(w)
    for win in [one] + shards:
        assert win.prepass(*values, jacobians=True)
    for fam, i in all_ids(one):
        t = (kp if fam == KP else gt)[i]
        owner = 0 if t["kind"] == "scale_prior" else [t["edge"] in capi.shard_edges(len(w.links), r, 2) for r in range(2)].index(True)
        rc, _ = serve(shards[1 - owner], fam, i, 0, check=False)
        assert rc == INVALID and serve_error(shards[1 - owner], fam, i, check=False)[0] == INVALID
        got, ref = serve(shards[owner], fam, i, 0), serve(one, fam, i, 0)
        assert got[3] == ref[3] and got[2] == ref[2]
        assert all(got[0][k].tobytes() == ref[0][k].tobytes() for k in ref[0])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1], ref[1]))
        assert serve_error(shards[owner], fam, i) == serve_error(one, fam, i)
    # a rank prepares its own terms only, on the host and on the device
    group = {(KP, 0): 0, (KP, 1): 1, (KP, 2): 2, (GRAPH, 0): 2, (GRAPH, 1): 2, (GRAPH, 2): 2}
    for sh in shards:
        own = [(fam, i) for fam, i in all_ids(sh) if serve_error(sh, fam, i, check=False)[0] == 0]
        groups = {group[(fam, family_kind(capi, sh, fam, i))] for fam, i in own}
        systems = systems_now(sh, own)
        sh.prepare_factors(1, 2)
        assert_serves_exactly(capi, sh, CS, systems, (1,))
        sh.prepare_factors_device()                                          # prepared already by the host call
        assert sh.prepare_factors_device_launches() == 0
        sh.prepare_factors(0, 1)
        worst = sh.prepare_factors_device()
        assert worst.status == 0 and sh.prepare_factors_device_launches() == 2 + len(groups)
        assert_serves_within_the_bar(capi, sh, CS, systems, "shard")
        sh.close()
    one.close()


# ------------------------------------------------------------------------------------------- 7. misuse
def test_misuse_is_answered_with_status_codes(capi):
    CS = 16
    w = make(CS)
    kp, gt = group2_terms(w)
    win = capi.Window(w, keypoint_terms=kp, graph_terms=gt)
    for fam, n in ((KP, len(kp)), (GRAPH, len(gt))):
        assert serve(win, fam, 0, 1, check=False)[0] == STATE               # before any prepass
        assert serve_error(win, fam, 0, check=False)[0] == STATE
        for bad in (-1, n):
            assert serve(win, fam, bad, 1, check=False)[0] == INVALID
            assert serve_error(win, fam, bad, check=False)[0] == INVALID
    assert win.prepass(*moved_values(w), jacobians=True)
    L = capi.lib()
    G = np.zeros(14 * 14, np.float64); g = np.zeros(14, np.float64); f = C.c_double()
    for name in ("sage_window_keypoint_factor", "sage_window_graph_factor"):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(win.h, 0, 1, G.ctypes.data, g.ctypes.data, None, None, None) == 0          # f, dims, nkeys are optional
        assert fn(win.h, 0, 1, None, g.ctypes.data, C.addressof(f), None, None) == INVALID
        assert fn(win.h, 0, 1, G.ctypes.data, None, C.addressof(f), None, None) == INVALID
        assert fn(win.h, 0, 3, G.ctypes.data, g.ctypes.data, None, None, None) == INVALID
        assert fn(win.h, 0, -1, G.ctypes.data, g.ctypes.data, None, None, None) == INVALID
        assert fn(None, 0, 1, G.ctypes.data, g.ctypes.data, None, None, None) == INVALID
    for name in ("sage_window_keypoint_factor_error", "sage_window_graph_factor_error"):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert fn(win.h, 0, None) == INVALID and fn(None, 0, C.addressof(f)) == INVALID
        assert fn(win.h, 0, C.addressof(f)) == 0 and f.value > 0
    # a window without terms has no term to serve, before and after a prepass
    plain = capi.Window(w)
    assert serve(plain, KP, 0, 1, check=False)[0] == INVALID and serve(plain, GRAPH, 0, 1, check=False)[0] == INVALID
    assert plain.prepass(*moved_values(w), jacobians=True)
    assert serve(plain, KP, 0, 1, check=False)[0] == INVALID and serve_error(plain, GRAPH, 0, check=False)[0] == INVALID
    win.close(); plain.close()
