"""Host side of the entry-by-entry system metric (tests/system_metric.py): the case tables the GPU parity suites run, their
scene builders and the oracle calls in either precision.  No GPU, no engine library: tests/test_system_metric.py measures
on these, with the oracle alone, the fp32 oracle's own distance from the fp64 oracle (the families' constants) and shows
that the metric sees the mutants the whole-matrix norm misses; the GPU suites take the same scenes.

``family_cases(orc, family)`` yields (label, segments, fp32 result, fp64 result) for every system of a family."""
import types

import numpy as np

from sage_slam_amd import capi, synth          # (capi: its host-side numpy helpers; the engine library is not loaded)
from tests import edge_scenes as es
from tests import system_metric as sm
from tests.helpers import oracle_geo, oracle_photo, presample_source

# per-edge dense operators (tests/test_gpu_parity.py: photometric on all five, geometric on the first four)
CASES = [
    dict(K=2, H=32, W=40, FS=16, CS=32, L=3, n_samples=0, seed=1),      # dense, N=384 (ragged last tile)
    dict(K=2, H=64, W=80, FS=16, CS=16, L=4, n_samples=3072, seed=2),   # reference defaults (slam_run.flags)
    dict(K=2, H=64, W=80, FS=16, CS=32, L=4, n_samples=700, seed=3),    # sampled, N % 256 != 0
    dict(K=2, H=32, W=40, FS=32, CS=32, L=2, n_samples=50, seed=4),     # N < one wave; FS=32
    dict(K=2, H=64, W=80, FS=32, CS=16, L=4, n_samples=0, seed=5),      # dense N=2400+
]
GEO_CASES = CASES[:4]


def case_id(c):
    return f"{c['H']}x{c['W']}_FS{c['FS']}_CS{c['CS']}_L{c['L']}_N{c['n_samples']}"


def masked_window():
    """destination mask with holes + some samples behind the camera (test_partially_masked_and_negative_depth)"""
    w = synth.make_window(K=2, H=64, W=80, FS=16, CS=32, L=4, n_samples=1000, seed=9)
    rng = np.random.default_rng(0)
    w.mask = (w.mask * (rng.uniform(size=w.mask.shape) < 0.8)).astype(np.float32)
    w.keyframes[0].bias[w.keyframes[0].loc1d[::7]] = -0.4        # negative depth for every 7th sample
    return w


# windows whose every directed edge goes against the oracle: name -> make_window arguments
WINDOWS = {
    "assembly_CS16": dict(K=5, H=64, W=80, FS=16, CS=16, L=4, seed=21, back_links=2),
    "assembly_CS32": dict(K=5, H=64, W=80, FS=16, CS=32, L=4, seed=21, back_links=2),
    "fs32_CS16": dict(K=3, H=64, W=80, FS=32, CS=16, L=4, seed=71, back_links=2),    # engine-layout FS = 32 kernels, small
    "fs32_CS32": dict(K=3, H=64, W=80, FS=32, CS=32, L=4, seed=72, back_links=2),
    "merged_pairs": dict(K=4, H=48, W=64, FS=16, CS=32, L=3, n_samples=2000, seed=41),
    "border_64x80": dict(K=4, H=64, W=80, FS=16, CS=32, L=4, seed=51, border=0, erode=0, pose_noise=2.0, back_links=3),
    "border_128x160": dict(K=4, H=128, W=160, FS=16, CS=32, L=4, seed=52, border=0, erode=0, pose_noise=2.0, back_links=3),
    "mixed_sampler": dict(K=4, H=128, W=160, FS=16, CS=32, L=4, seed=61, border=2, erode=5, pose_noise=2.0, back_links=3),
}
MIXED_SAMPLER_DZ = [0.0, 0.2, 0.03, 0.27]
FULL_SIZE = [dict(K=4, H=128, W=160, FS=16, CS=32), dict(K=3, H=256, W=320, FS=32, CS=32)]      # L = 4, seed = 41: edge 0 only


def make_named_window(name):
    w = synth.make_window(**WINDOWS[name])
    if name == "mixed_sampler":
        for k, z in enumerate(MIXED_SAMPLER_DZ):
            w.keyframes[k].t[2] += np.float32(z)
    return w


def directed_edges(w):
    return [(k0, k1) for (a, b) in w.links for (k0, k1) in ((a, b), (b, a))]


def window_oracle(orc, w, prec):
    """{(type, link, direction): oracle result} of every directed edge, both factor types"""
    res = {}
    for l, (a, b) in enumerate(w.links):
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            res[(0, l, d)] = oracle_photo(orc, w, k0, k1, prec=prec)
            res[(1, l, d)] = oracle_geo(orc, w, k0, k1, prec=prec)
    return res


_WINDOW_ORACLE = {}


def named_window_oracle(orc, name, prec):
    """window_oracle of a window of the table, computed once per session (the per-edge families and the window family
    share it; the results are not to be changed)"""
    if (name, prec) not in _WINDOW_ORACLE:
        _WINDOW_ORACLE[(name, prec)] = window_oracle(orc, make_named_window(name), prec)
    return _WINDOW_ORACLE[(name, prec)]


def combined_pair(p, g, CS):
    """photometric + geometric result of one directed pair in the geometric edge's index space -> dict(AtA, Atb), fp64"""
    emb = np.concatenate([np.arange(12 + CS), [12 + 2 * CS]])          # photometric column -> geometric column
    A = np.array(g["AtA"], np.float64); v = np.array(g["Atb"], np.float64)
    A[np.ix_(emb, emb)] += np.asarray(p["AtA"], np.float64); v[emb] += np.asarray(p["Atb"], np.float64)
    return dict(AtA=A, Atb=v)


def dense_system(packed, K, links, CS):
    """the packed layout [diag | link | g | tail] -> dict(AtA [K*B, K*B], Atb [K*B]), fp64"""
    H, g, _ = capi.unpack_dense(np.asarray(packed, np.float64), K, links, CS)
    return dict(AtA=H, Atb=g)


# ---------------------------------------------------------------------------------------------------------------------
# keypoint per-edge factors (tests/test_gpu_parity.py)
# ---------------------------------------------------------------------------------------------------------------------
REPROJ_CASES = [(32, 300), (16, 129), (32, 1), (16, 1000)]
MATCH_GEOM_CASES = [(32, 257), (16, 40), (16, 700)]
MG_LOSSES = ("fair", "L2", "huber", "unbiased")


# The scene's seed is 100 + N, except (32, 300): at seed 400 the pose x code-high correlations of the nominal variant are so
# small that mutant (c) of tests/test_system_metric.py is 9.8 bars away where 10 are asked; 500 is the next seed tried (16.8).
REPROJ_SEEDS = {(32, 300): 500}


def reproj_scene(CS, N):
    rng = np.random.default_rng(REPROJ_SEEDS.get((CS, N), 100 + N))
    H, W = 64, 80
    cam = synth.Camera(72.0, 70.5, 39.5, 31.5, float(W), float(H))
    bias0 = (1.0 + 0.2 * rng.random(H * W)).astype(np.float32)
    basis0 = (0.05 * rng.standard_normal((H * W, CS))).astype(np.float32)
    code0 = (0.3 * rng.standard_normal(CS)).astype(np.float32); s0 = 1.1
    ys = rng.integers(0, H, N); xs = rng.integers(0, W, N)
    loc = (ys * W + xs).astype(np.int32)
    homo = np.stack([(xs - cam.cx) / cam.fx, (ys - cam.cy) / cam.fy, np.ones(N)], 1).astype(np.float32)
    R0 = synth.so3_exp(np.array([0.03, -0.05, 0.02])).astype(np.float32); t0 = np.array([0.02, -0.01, 0.03], np.float32)
    R1 = synth.so3_exp(np.array([-0.02, 0.04, 0.06])).astype(np.float32); t1 = np.array([-0.04, 0.02, -0.03], np.float32)
    R10 = (R1.T @ R0).astype(np.float32); t10 = (R1.T @ (t0 - t1)).astype(np.float32)
    d0 = s0 * (bias0[loc] + basis0[loc] @ code0)
    X = (R10 @ (d0[:, None] * homo).T).T + t10
    matched = (np.stack([X[:, 0] / X[:, 2] * cam.fx + cam.cx, X[:, 1] / X[:, 2] * cam.fy + cam.cy], 1)
               + rng.normal(0, 2.0, (N, 2))).astype(np.float32)
    return types.SimpleNamespace(CS=CS, N=N, H=H, W=W, cam=cam, bias0=bias0, basis0=basis0, code0=code0, s0=s0, loc=loc,
                                 homo=homo, R0=R0, t0=t0, R1=R1, t1=t1, R10=R10, t10=t10, matched=matched,
                                 eps=1e-4, c=1.7, wgt=0.4)


def reproj_variants(s):
    """[(name, t10, bias)]: "some_behind" flips a few depths through the bias, "all_behind" moves the camera away"""
    out = [("nominal", s.t10, s.bias0.copy())]
    if s.N > 1:
        b = s.bias0.copy()
        b[s.loc[::3]] = -5.0                      # negative depth -> behind the camera
        out.append(("some_behind", s.t10, b))
        out.append(("all_behind", (s.t10 - np.array([0, 0, 100.0])).astype(np.float32), s.bias0.copy()))
    return out


def oracle_reproj(orc, s, tt, b, prec="f32"):
    return orc.reproj_jac_error(s.R10, tt, s.R0, s.t0, s.R1, s.t1, b, s.basis0, s.code0, s.loc, s.homo, s.matched, s.s0,
                                s.cam, s.eps, s.c, s.wgt, prec=prec)


def oracle_tracker_reproj(orc, s, tt, b, prec="f32"):
    dd = (s.s0 * (b[s.loc] + s.basis0[s.loc] @ s.code0)).astype(np.float32)
    return orc.tracker_reproj_jac_error(s.R10, tt, dd, s.homo, s.matched, s.cam, s.eps, s.c, s.wgt, prec=prec)


def match_geom_scene(CS, N):
    rng = np.random.default_rng(300 + N)
    HW = 2000
    bias0 = (1.0 + 0.2 * rng.random(HW)).astype(np.float32); bias1 = (1.1 + 0.2 * rng.random(HW)).astype(np.float32)
    basis0 = (0.05 * rng.standard_normal((HW, CS))).astype(np.float32)
    basis1 = (0.05 * rng.standard_normal((HW, CS))).astype(np.float32)
    code0 = (0.3 * rng.standard_normal(CS)).astype(np.float32); code1 = (0.3 * rng.standard_normal(CS)).astype(np.float32)
    s0, s1 = 1.2, 0.9
    loc0 = rng.integers(0, HW, N).astype(np.int32); loc1 = rng.integers(0, HW, N).astype(np.int32)
    homo0 = np.concatenate([rng.uniform(-0.5, 0.5, (N, 2)), np.ones((N, 1))], 1).astype(np.float32)
    homo1 = np.concatenate([rng.uniform(-0.5, 0.5, (N, 2)), np.ones((N, 1))], 1).astype(np.float32)
    R0 = synth.so3_exp(np.array([0.03, -0.05, 0.02])).astype(np.float32); t0 = np.array([0.02, -0.01, 0.03], np.float32)
    R1 = synth.so3_exp(np.array([-0.02, 0.04, 0.06])).astype(np.float32); t1 = np.array([-0.04, 0.02, -0.03], np.float32)
    R10 = (R1.T @ R0).astype(np.float32); t10 = (R1.T @ (t0 - t1)).astype(np.float32)
    u0 = (bias0[loc0] + basis0[loc0] @ code0).astype(np.float32); u1 = (bias1[loc1] + basis1[loc1] @ code1).astype(np.float32)
    d0 = (s0 * u0).astype(np.float32); d1 = (s1 * u1).astype(np.float32)
    hz0 = homo0.copy(); hz0[:, 0] = 0.0
    hz1 = homo1.copy(); hz1[:, 0] = 0.0
    return types.SimpleNamespace(CS=CS, N=N, bias0=bias0, bias1=bias1, basis0=basis0, basis1=basis1, code0=code0, code1=code1,
                                 s0=s0, s1=s1, loc0=loc0, loc1=loc1, homo0=homo0, homo1=homo1, R0=R0, t0=t0, R1=R1, t1=t1,
                                 R10=R10, t10=t10, u0=u0, u1=u1, d0=d0, d1=d1, hz0=hz0, hz1=hz1, c=0.05, wgt=0.8)


def oracle_match_geom(orc, s, loss, prec="f32"):
    return orc.match_geom_jac_error(0, loss, s.R10, s.t10, s.R0, s.t0, s.R1, s.t1, s.bias0, s.bias1, s.basis0, s.basis1,
                                    s.code0, s.code1, homo0=s.homo0, homo1=s.homo1, loc0=s.loc0, loc1=s.loc1, scale0=s.s0,
                                    scale1=s.s1, loss_param=s.c, weight=s.wgt, prec=prec)


def oracle_loop_mg(orc, s, prec="f32"):
    return orc.match_geom_jac_error(1, "fair", s.R10, s.t10, s.R0, s.t0, s.R1, s.t1, dpts0=s.u0, dpts1=s.u1, homo0=s.homo0,
                                    homo1=s.homo1, scale0=s.s0, scale1=s.s1, loss_param=s.c, weight=s.wgt, prec=prec)


def oracle_tracker_mg(orc, s, mode, prec="f32"):
    return orc.match_geom_jac_error(mode, "fair", s.R10, s.t10, dpts0=s.d0, dpts1=s.d1, homo0=s.homo0, homo1=s.homo1,
                                    scale0=s.s0, loss_param=s.c, weight=s.wgt, prec=prec)


def oracle_huber_zero(orc, s, prec="f32"):
    """huber with an exactly-zero difference component (x = 0 on both sides, identity pose)"""
    I3 = np.eye(3, dtype=np.float32); z3 = np.zeros(3, np.float32)
    return orc.match_geom_jac_error(0, "huber", I3, z3, I3, z3, I3, z3, s.bias0, s.bias1, s.basis0, s.basis1, s.code0, s.code1,
                                    homo0=s.hz0, homo1=s.hz1, loc0=s.loc0, loc1=s.loc1, scale0=s.s0, scale1=s.s1,
                                    loss_param=s.c, weight=s.wgt, prec=prec)


# ---------------------------------------------------------------------------------------------------------------------
# the tracker's photometric operator: the BASELINE config-1 scene of test_tracker_linearize_and_error
# ---------------------------------------------------------------------------------------------------------------------
def tracker_parity_scene():
    w = synth.make_window(K=2, H=64, W=80, FS=16, CS=32, L=4, n_samples=3072, seed=11)
    a, b = w.keyframes[0], w.keyframes[1]
    R10, t10 = synth.relative_pose(a.R, a.t, b.R, b.t)
    feat0s = presample_source(None, w, a)
    dpts0 = (np.float32(a.scale) * (a.bias + a.basis @ a.code))[a.loc1d].astype(np.float32)
    return types.SimpleNamespace(w=w, a=a, b=b, R10=R10, t10=t10, feat0s=feat0s, dpts0=dpts0)


def oracle_tracker_photo(orc, s, dof, prec="f32"):
    w, a, b = s.w, s.a, s.b
    return orc.tracker_photo_jac_error(dof, s.R10, s.t10, w.mask, s.dpts0, a.homo, s.feat0s, b.feat_pyr, b.grad_pyr,
                                       w.level_offsets, w.cams, w.eps, w.photo_weights, scale0=a.scale, prec=prec)


# ---------------------------------------------------------------------------------------------------------------------
# every system of a family, fp32 and fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def _pairs(orc, fn, *args):
    return fn(orc, *args, prec="f32"), fn(orc, *args, prec="f64")


def _window_edges(orc, t):
    for name in WINDOWS:
        w = make_named_window(name)
        r32, r64 = named_window_oracle(orc, name, "f32"), named_window_oracle(orc, name, "f64")
        for e, (k0, k1) in enumerate(directed_edges(w)):
            key = (t, e // 2, e % 2)
            yield f"window {name} {k0}->{k1}", (sm.seg_geo if t else sm.seg_photo)(w.CS), r32[key], r64[key]


def _photometric(orc):
    for c in CASES:
        w = synth.make_window(**c)
        for k0, k1 in ((0, 1), (1, 0)):
            yield f"{case_id(c)} {k0}->{k1}", sm.seg_photo(c["CS"]), *_pairs(orc, oracle_photo, w, k0, k1)
    yield "masked 0->1", sm.seg_photo(32), *_pairs(orc, oracle_photo, masked_window(), 0, 1)
    yield from _window_edges(orc, 0)
    for c in FULL_SIZE:
        w = synth.make_window(L=4, seed=41, **c)
        yield f"full size {c['H']}x{c['W']} 0->1", sm.seg_photo(c["CS"]), *_pairs(orc, oracle_photo, w, 0, 1)


def _geometric(orc):
    for c in GEO_CASES:
        w = synth.make_window(**c)
        for k0, k1 in ((0, 1), (1, 0)):
            yield f"{case_id(c)} {k0}->{k1}", sm.seg_geo(c["CS"]), *_pairs(orc, oracle_geo, w, k0, k1)
    yield "masked 0->1", sm.seg_geo(32), *_pairs(orc, oracle_geo, masked_window(), 0, 1)
    yield from _window_edges(orc, 1)
    for c in FULL_SIZE:
        w = synth.make_window(L=4, seed=41, **c)
        yield f"full size {c['H']}x{c['W']} 0->1", sm.seg_geo(c["CS"]), *_pairs(orc, oracle_geo, w, 0, 1)


def _merged_pair(orc):
    for name in ("merged_pairs", "fs32_CS16", "fs32_CS32"):
        w = make_named_window(name)
        for e, (k0, k1) in enumerate(directed_edges(w)):
            r = [combined_pair(named_window_oracle(orc, name, p)[(0, e // 2, e % 2)], named_window_oracle(orc, name, p)[(1, e // 2, e % 2)],
                               w.CS) for p in ("f32", "f64")]
            yield f"{name} pair {k0}->{k1}", sm.seg_geo(w.CS), *r


def _window(orc):
    for name in WINDOWS:
        if name == "merged_pairs":
            continue
        w = make_named_window(name)
        K = len(w.keyframes)
        r = [dense_system(capi.assemble_packed(K, w.links, w.CS, named_window_oracle(orc, name, p)), K, w.links, w.CS)
             for p in ("f32", "f64")]
        yield f"window {name}", sm.seg_window(K, w.CS), *r


def _reprojection(orc):
    for CS, N in REPROJ_CASES:
        s = reproj_scene(CS, N)
        for name, tt, b in reproj_variants(s):
            if name != "all_behind":
                yield f"CS{CS}_N{N} {name}", sm.seg_photo(CS), *_pairs(orc, oracle_reproj, s, tt, b)


def _window_terms(orc, kind):
    """the keypoint terms of tests/test_gpu_window_keypoints.py (its host-side builders; importing it starts no GPU work)"""
    from tests import test_gpu_window_keypoints as wk
    sets = [(f"CS{CS} {loss}", wk.make(CS), loss) for CS, loss in wk.TERM_CASES] + [("chunks", wk.make(), None)]
    for label, w, loss in sets:
        terms = wk.chunk_terms(w) if loss is None else wk.all_terms(w, rep=(loss == "fair"), mg_loss=loss)
        xs = wk.initial_vars(w)
        for i, t in enumerate(terms):
            if t["kind"] == kind:
                segs = sm.seg_photo(w.CS) if kind == "reprojection" else sm.seg_geo(w.CS)
                yield (f"window term {label} #{i} edge {t['edge']}", segs, wk.oracle_term(orc, w, t, xs),
                       wk.oracle_term(orc, w, t, xs, prec="f64"))


def _tracker_reprojection(orc):
    for CS, N in REPROJ_CASES:
        s = reproj_scene(CS, N)
        for name, tt, b in reproj_variants(s):
            if name != "all_behind":
                yield f"CS{CS}_N{N} {name}", sm.seg_tracker(6), *_pairs(orc, oracle_tracker_reproj, s, tt, b)


def _match_geometry(orc):
    for CS, N in MATCH_GEOM_CASES:
        s = match_geom_scene(CS, N)
        for loss in MG_LOSSES:
            yield f"CS{CS}_N{N} {loss}", sm.seg_geo(CS), *_pairs(orc, oracle_match_geom, s, loss)
        yield f"CS{CS}_N{N} huber zero difference", sm.seg_geo(CS), *_pairs(orc, oracle_huber_zero, s)


def _loop_mg(orc):
    for CS, N in MATCH_GEOM_CASES:
        yield f"CS{CS}_N{N}", sm.seg_loop(), *_pairs(orc, oracle_loop_mg, match_geom_scene(CS, N))


def _tracker_match_geometry(orc):
    for CS, N in MATCH_GEOM_CASES:
        s = match_geom_scene(CS, N)
        for mode in (2, 3):
            yield f"CS{CS}_N{N} mode {mode}", sm.seg_tracker(4 + mode), *_pairs(orc, oracle_tracker_mg, s, mode)


def _tracker_photometric(orc):
    s = tracker_parity_scene()
    for dof in (6, 7):
        yield f"config 1 dof {dof}", sm.seg_tracker(dof), *_pairs(orc, oracle_tracker_photo, s, dof)
    for c in es.TRACKER_CASES:
        sc = es.tracker_scene(**c)
        for dof in (6, 7):
            yield f"{es.tracker_case_id(c)} dof {dof}", sm.seg_tracker(dof), es.oracle_jac(orc, sc, dof), es.oracle_jac(orc, sc, dof, "f64")


def _graph_terms(orc):
    """the window's graph terms (D = 14): the fp32 restatement against the fp64 one (tests/graph_term_ref.py; no oracle call)"""
    from tests import graph_term_ref as G
    from tests import test_gpu_window_graph_terms as gt
    for label, w, links, terms in gt.parity_term_sets():
        for i, c in enumerate(gt.cases_of(w, links, terms)):
            yield f"{label} #{i} {terms[i]['kind']}", sm.seg_loop(), G.linearize(*c, dtype=np.float32), G.linearize(*c)


FAMILIES = {
    "photometric": _photometric,
    "geometric": _geometric,
    "merged_pair": _merged_pair,
    "window": _window,
    "reprojection": _reprojection,
    "tracker_reprojection": _tracker_reprojection,
    "match_geometry": _match_geometry,
    "loop_mg": _loop_mg,
    "tracker_match_geometry": _tracker_match_geometry,
    "tracker_photometric": _tracker_photometric,
    "window_reprojection": lambda orc: _window_terms(orc, "reprojection"),
    "window_match_geometry": lambda orc: _window_terms(orc, "match_geometry"),
    "graph_terms": _graph_terms,
}


def family_cases(orc, family):
    return FAMILIES[family](orc)
