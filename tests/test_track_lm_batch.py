"""sage_track_lm_batch (csrc/host_math.cpp): B runs of the tracker's LM policy in lock-step, and the device-free half of
sage_track_frame_batch / sage_loop_verify: the header declares them, the library exports them, their argument checks answer
before anything touches a device.

sage_track_lm and sage_track_lm_batch drive ONE stepper, and the callbacks of these tests are deterministic (the fp32 oracle
composed as HostScene.oracle_callbacks composes it): row b of a batch must equal the single run byte for byte -- pose, scale,
error, iterations, status and every trace entry -- for trajectories of different length and branch in one batch.  The batch
callback must see every live problem exactly once per round, in ascending order, and never a finished one."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import edge_scenes as es
from tests import track_batch_cases as tb
from tests.tracker_scene import HostScene
from tests.test_lm_trace_golden import check_trace, product_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID, SAGE_E_NO_OVERLAP = -1, -5
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "lm_trace_*.json")))


# ---------------------------------------------------------------------------------------------------------------------
# declarations, exports, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in ("sage_track_lm_batch", "sage_track_frame_batch", "sage_loop_verify"):
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"#define SAGE_TRACK_MAX_BATCH (\d+)", hdr).group(1) == str(capi.SAGE_TRACK_MAX_BATCH) == "32"
    assert "typedef int (*SageTrackBatchEvalFn)" in hdr
    for s in ("SageLoopVerifyQuery", "SageLoopVerifyCandidate", "SageLoopVerifyResult"):
        assert "typedef struct " + s in hdr


class LmArgs:
    """a valid argument set of sage_track_lm_batch (B = 3) whose callback counts its calls: every case changes one thing"""

    def __init__(self):
        self.calls = 0

        def _eval(ctx, n, problem, want_jac, p, s, AtA, Atb, err):
            self.calls += 1
            return 7                                          # (ends the call at once, with this code)

        self.cb = capi.TRACK_BATCH_EVAL_FN(_eval)
        self.cfg = capi.lm_config_default()
        self.pose = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (32, 1))
        self.scale = np.ones(32, np.float32)
        self.status = np.full(32, 99, np.int32)

    def run(self, **kw):
        a = dict(cfg=C.addressof(self.cfg), dof=7, B=3, cb=self.cb, pose=self.pose.ctypes.data, scale=self.scale.ctypes.data,
                 status=self.status.ctypes.data)
        a.update(kw)
        return capi.track_lm_batch_raw(a["cfg"], a["dof"], a["B"], a["cb"], a["pose"], a["scale"], None, None, a["status"], None, 0,
                                       None)


@pytest.mark.parametrize("change", [dict(cfg=None), dict(cb=None), dict(pose=None), dict(status=None), dict(dof=5), dict(dof=8),
                                    dict(scale=None), dict(B=-1), dict(B=33)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_lm_batch_refuses_invalid_arguments(change):
    a = LmArgs()
    assert a.run(**change) == SAGE_E_INVALID
    assert a.calls == 0 and (a.status == 99).all()


def test_lm_batch_empty_batch_and_callback_failure():
    a = LmArgs()
    assert a.run(B=0) == 0 and a.calls == 0                   # B = 0: SAGE_OK, nothing called
    assert a.run(B=0, pose=None, status=None, scale=None) == SAGE_E_INVALID
    assert a.run(dof=6, scale=None) == 7 and a.calls == 1     # dof 6 needs no scale; a non-zero return of eval ends the call
    assert a.run(B=32) == 7 and a.calls == 2
    assert (a.status == 99).all()


class FrameArgs:
    """a valid argument set of sage_track_frame_batch (B = 2, dof 7, both terms) whose pointers are never followed"""

    def __init__(self):
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        self.cfg = capi.lm_config_default()
        self.probs = (capi.SageTrackProblem * 32)()
        p = C.addressof(self.dummy)
        cam = capi.SageCamera(60.0, 60.0, 3.5, 3.5, 8.0, 8.0)
        for pr in self.probs:
            pr.ws = C.addressof(self.ws)
            pr.use_photo = pr.use_keypoints = 1
            for f in ("mask1_dev", "dpts0_dev", "homo_dev", "feat0s_dev", "feat1_dev", "grad1_dev", "weights_dev", "kp_dpts0_dev",
                      "kp_homo0_dev", "kp_matched_2d_dev", "kp_matched_dpts1_dev", "kp_matched_homo1_dev"):
                setattr(pr, f, p)
            pr.pyr.levels = 1; pr.pyr.P = 64; pr.pyr.cam[0] = cam
            pr.eps = 1e-6; pr.N = 5; pr.FS = 16; pr.NK = 4
        self.pose = np.zeros((32, 12), np.float32); self.scale = np.ones(32, np.float32)
        self.status = np.full(32, 99, np.int32)

    def run(self, **kw):
        a = dict(cfg=C.addressof(self.cfg), dof=7, probs=C.addressof(self.probs), B=2, pose=self.pose.ctypes.data,
                 scale=self.scale.ctypes.data, status=self.status.ctypes.data)
        a.update(kw)
        return capi.track_frame_batch_raw(a["cfg"], a["dof"], a["probs"], a["B"], a["pose"], a["scale"], None, None, a["status"],
                                          None, 0, None)


def _set(field, value, b=1):
    def f(a):
        obj = a.probs[b]
        *path, last = field.split(".")
        for k in path:
            obj = getattr(obj, k)
        setattr(obj, last, value)
    return f


FRAME_INVALID = [("cfg", dict(cfg=None)), ("probs", dict(probs=None)), ("pose", dict(pose=None)), ("status", dict(status=None)),
                 ("scale", dict(scale=None)), ("dof5", dict(dof=5)), ("B-1", dict(B=-1)), ("B33", dict(B=33)),
                 ("null-ws", _set("ws", None)), ("no-term", lambda a: [_set("use_photo", 0, b)(a) or _set("use_keypoints", 0, b)(a) for b in (0, 1)]),
                 ("null-feat1", _set("feat1_dev", None)), ("N0", _set("N", 0)), ("NK0", _set("NK", 0)),
                 ("null-homo1", _set("kp_matched_homo1_dev", None)),
                 ("other-ws", lambda a: _set("ws", C.addressof(a.dummy))(a)), ("other-FS", _set("FS", 32)),
                 ("other-use_photo", _set("use_photo", 0)), ("other-use_keypoints", _set("use_keypoints", 0)),
                 ("other-eps", _set("eps", 2e-6)), ("other-levels", _set("pyr.levels", 2)), ("other-P", _set("pyr.P", 65)),
                 ("other-camera", lambda a: setattr(a.probs[1].pyr.cam[0], "fx", 61.0))]


@pytest.mark.parametrize("change", [c for _, c in FRAME_INVALID], ids=[n for n, _ in FRAME_INVALID])
def test_frame_batch_refuses_invalid_arguments_without_a_device(change):
    a = FrameArgs()
    kw = change if isinstance(change, dict) else (change(a) and {}) or {}
    assert a.run(**kw) == SAGE_E_INVALID
    assert (a.status == 99).all()


def test_frame_batch_empty_batch():
    a = FrameArgs()
    assert a.run(B=0) == 0 and a.run(B=0, probs=None) == 0
    a.probs[5].ws = None                                       # (a problem past B is not looked at)
    assert a.run(B=0) == 0


class VerifyArgs:
    """a valid argument set of sage_loop_verify (B = 3, K = 8; candidate 0 a survivor) whose pointers are never followed"""

    def __init__(self):
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        p = self.p = C.addressof(self.dummy)
        self.cfg = capi.lm_config_default()
        q = self.query = capi.SageLoopVerifyQuery()
        q.N = 10; q.FS = 16; q.M = 12; q.eps = 1e-6
        for f in ("homo_dev", "unscaled_dpts0_dev", "feat0s_dev", "weights_dev", "valid_homo_dev", "valid_dpts0_dev", "mask_dev"):
            setattr(q, f, p)
        q.pyr.levels = 1; q.pyr.P = 64; q.pyr.cam[0] = capi.SageCamera(60.0, 60.0, 3.5, 3.5, 8.0, 8.0)
        self.cands = (capi.SageLoopCandidate * 32)(*[capi.SageLoopCandidate(p, p, p, p, p) for _ in range(32)])
        self.vcands = (capi.SageLoopVerifyCandidate * 32)(*[capi.SageLoopVerifyCandidate(p, p, p, 0.1) for _ in range(32)])
        self.pre = (capi.SageLoopPrecheckResult * 32)()
        self.pre[0].registered = 1; self.pre[0].reg.n_inliers = 5
        self.results = (capi.SageLoopVerifyResult * 32)()
        for r in self.results:
            r.tracked = 77

    def run(self, divisor=1.0, **kw):
        a = dict(ws=C.addressof(self.ws), cfg=C.addressof(self.cfg), query=C.addressof(self.query), cands=C.addressof(self.cands),
                 vcands=C.addressof(self.vcands), pre=C.addressof(self.pre), B=3, K=8, raw=self.p, ikp=self.p, gathered=self.p,
                 results=C.addressof(self.results))
        a.update(kw)
        return capi.loop_verify_raw(a["ws"], a["cfg"], a["query"], divisor, a["cands"], a["vcands"], a["pre"], a["B"], a["K"], a["raw"],
                                    a["ikp"], 3.0, a["gathered"], a["results"])


def _q(field, value):
    return lambda a: setattr(a.query, field, value)


VERIFY_INVALID = [("ws", dict(ws=None)), ("cfg", dict(cfg=None)), ("query", dict(query=None)), ("results", dict(results=None)),
                  ("B-1", dict(B=-1)), ("B33", dict(B=33)), ("K-1", dict(K=-1)), ("K1025", dict(K=1025)), ("cands", dict(cands=None)),
                  ("vcands", dict(vcands=None)), ("pre", dict(pre=None)), ("raw", dict(raw=None)), ("ikp", dict(ikp=None)),
                  ("gathered", dict(gathered=None)), ("divisor0", dict(divisor=0.0)), ("divisor-nan", dict(divisor=float("nan"))),
                  ("N0", _q("N", 0)), ("M0", _q("M", 0)), ("FS8", _q("FS", 8)), ("null-feat0s", _q("feat0s_dev", None)),
                  ("null-mask", _q("mask_dev", None)), ("levels0", lambda a: setattr(a.query.pyr, "levels", 0)),
                  ("fx0", lambda a: setattr(a.query.pyr.cam[0], "fx", 0.0)),
                  ("survivor-null-feat1", lambda a: setattr(a.vcands[0], "feat1_dev", None)),
                  ("survivor-null-dpt_map", lambda a: setattr(a.cands[0], "dpt_map_dev", None)),
                  ("survivor-inliers>K", lambda a: setattr(a.pre[0].reg, "n_inliers", 9))]


@pytest.mark.parametrize("change", [c for _, c in VERIFY_INVALID], ids=[n for n, _ in VERIFY_INVALID])
def test_loop_verify_refuses_invalid_arguments_without_a_device(change):
    a = VerifyArgs()
    kw = change if isinstance(change, dict) else (change(a) and {}) or {}
    assert a.run(**kw) == SAGE_E_INVALID
    assert all(r.tracked == 77 for r in a.results)


def test_loop_verify_without_survivors_zeroes_the_results():
    a = VerifyArgs()
    assert a.run(B=0) == 0 and all(r.tracked == 77 for r in a.results)
    a.pre[0].reg.n_inliers = 3                                 # <= 3 registration inliers: not tracked (camera_tracker.cpp:1407)
    a.pre[1].registered = 0; a.pre[1].reg.n_inliers = 8        # pruned by the ratio
    a.vcands[1].feat1_dev = None                               # (a non-survivor's members are not looked at)
    assert a.run() == 0
    assert all(r.tracked == 0 for r in a.results[:3]) and a.results[3].tracked == 77


# ---------------------------------------------------------------------------------------------------------------------
# the policy: a batch against its singles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(orc):
    return HostScene(orc, **es.LM_SCENE)


def single_lm(cfg, dof, lin, err, pose, scale, trace_cap=256):
    """one sage_track_lm run with the C outputs as they are -> (rc, pose, scale, error, iters, trace, the callback kinds)"""
    kinds = []

    def _lin(ctx, p, s, AtA, Atb, e):
        kinds.append(1)
        A, b, v = lin(np.ctypeslib.as_array(p, (12,)).copy(), float(s))
        A = np.asarray(A, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
        for i in range(dof * dof):
            AtA[i] = A[i]
        for i in range(dof):
            Atb[i] = b[i]
        e[0] = v
        return 0

    def _err(ctx, p, s, e):
        kinds.append(0)
        e[0] = err(np.ctypeslib.as_array(p, (12,)).copy(), float(s))
        return 0

    p = np.asarray(pose, np.float32).copy()
    sc = C.c_float(scale); fe = C.c_float(); it = C.c_int(); tl = C.c_int()
    tr = (capi.SageLmTraceEntry * trace_cap)()
    rc = capi.lib().sage_track_lm(C.byref(cfg), dof, capi.TRACK_LIN_FN(_lin), capi.TRACK_ERR_FN(_err), None,
                                  p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(sc), C.byref(fe), C.byref(it), tr, trace_cap,
                                  C.byref(tl))
    return rc, p, np.float32(sc.value), np.float32(fe.value), it.value, capi._trace_dicts(tr, tl.value), kinds


def batch_eval(callbacks, record=None):
    """the batch callback over per-problem (lin, err) pairs; record: a list that receives (problems, want_jac) per call"""
    def ev(problems, want_jac, poses, scales):
        if record is not None:
            record.append((list(problems), list(want_jac)))
        out = []
        for i, (b, wj) in enumerate(zip(problems, want_jac)):
            lin, err = callbacks[b]
            out.append(lin(poses[i], float(scales[i])) if wj else err(poses[i], float(scales[i])))
        return out
    return ev


@pytest.mark.parametrize("capped", [False, True], ids=["default", "max_num_iters=2"])
@pytest.mark.parametrize("dof,use_photo,use_kp", tb.COMPOSITIONS, ids=tb.COMPOSITION_IDS)
def test_batch_equals_its_singles_byte_for_byte(scene, dof, use_photo, use_kp, capped):
    cfg = tb.configure(capi, scene, dof, use_photo, use_kp, capped)
    st = tb.starts(scene, dof, use_photo, use_kp)
    cb = scene.oracle_callbacks(dof, use_photo, use_kp)
    singles = [single_lm(cfg, dof, cb[0], cb[1], p, s) for p, s in st]
    # what the batch test rests on: trajectories that differ in length and in branch
    iters = [r[4] for r in singles]
    print("iterations", iters, "status", [r[0] for r in singles])
    assert all(r[0] in (0, SAGE_E_NO_OVERLAP) for r in singles)
    if not capped:
        assert len(set(iters)) >= 3
        assert any(not t["accepted"] for r in singles for t in r[5])               # a step rejected up to max_damp
        assert any(np.float32(t["damp"]) == np.float32(cfg.max_damp) for r in singles for t in r[5])
        assert iters[1] <= 1 and iters[0] > tb.CAP                                  # the early finisher; what the cap cuts
        if dof == 7 and not use_kp:                                                 # the no-overlap exit: pose untouched
            assert singles[3][0] == SAGE_E_NO_OVERLAP and iters[3] == 0 and np.array_equal(singles[3][1], st[3][0])
    else:
        assert iters[0] == tb.CAP and max(iters) == tb.CAP
    record = []
    rc, P, S, E, IT, ST, TR = capi.track_lm_batch(cfg, dof, batch_eval([cb] * len(st), record), [p for p, _ in st],
                                                  [s for _, s in st])
    assert rc == 0
    for b, r in enumerate(singles):
        tb.assert_row_equals_single((ST[b], P[b], S[b], E[b], IT[b], TR[b]), r[:6], f"problem {b}")
    # every live problem exactly once per round, ascending, never a finished one: problem b is in the first
    # len(its single run's callbacks) rounds and in no other, with the single run's sequence of request kinds
    assert all(pr == sorted(set(pr)) and len(pr) >= 1 for pr, _ in record)
    for b, r in enumerate(singles):
        seen = [(k, wj[pr.index(b)]) for k, (pr, wj) in enumerate(record) if b in pr]
        assert [k for k, _ in seen] == list(range(len(r[6]))), f"problem {b}"
        assert [int(j) for _, j in seen] == r[6], f"problem {b}"
    assert len(record) == max(len(r[6]) for r in singles)


def test_batch_of_one_and_order_of_the_problems(scene):
    dof, use_photo, use_kp = 7, True, True
    cfg = tb.configure(capi, scene, dof, use_photo, use_kp)
    st = tb.starts(scene, dof, use_photo, use_kp)
    cb = scene.oracle_callbacks(dof, use_photo, use_kp)
    _, P, S, E, IT, ST, TR = capi.track_lm_batch(cfg, dof, batch_eval([cb] * 5), [p for p, _ in st], [s for _, s in st])
    perm = [3, 0, 4, 2, 1]
    _, P2, S2, E2, IT2, ST2, TR2 = capi.track_lm_batch(cfg, dof, batch_eval([cb] * 5), [st[k][0] for k in perm],
                                                       [st[k][1] for k in perm])
    for i, k in enumerate(perm):
        tb.assert_row_equals_single((ST2[i], P2[i], S2[i], E2[i], IT2[i], TR2[i]), (ST[k], P[k], S[k], E[k], IT[k], TR[k]))
    _, P1, S1, E1, IT1, ST1, TR1 = capi.track_lm_batch(cfg, dof, batch_eval([cb]), [st[2][0]], [st[2][1]])
    tb.assert_row_equals_single((ST1[0], P1[0], S1[0], E1[0], IT1[0], TR1[0]), (ST[2], P[2], S[2], E[2], IT[2], TR[2]))


def test_trace_capacity_is_per_problem(scene):
    dof, use_photo, use_kp = 6, True, True
    cfg = tb.configure(capi, scene, dof, use_photo, use_kp)
    st = tb.starts(scene, dof, use_photo, use_kp)
    cb = scene.oracle_callbacks(dof, use_photo, use_kp)
    full = capi.track_lm_batch(cfg, dof, batch_eval([cb] * 5), [p for p, _ in st], [s for _, s in st])
    cut = capi.track_lm_batch(cfg, dof, batch_eval([cb] * 5), [p for p, _ in st], [s for _, s in st], trace_cap=2)
    for b in range(5):
        assert cut[6][b] == full[6][b][:2] and np.array_equal(cut[1][b], full[1][b]) and cut[4][b] == full[4][b]


# ---------------------------------------------------------------------------------------------------------------------
# the committed golden traces, a group per batch
# ---------------------------------------------------------------------------------------------------------------------
def golden_groups():
    groups = {}
    for path in GOLDEN:
        rec = json.load(open(path))
        groups.setdefault((rec["dof"], json.dumps(rec["config"], sort_keys=True)), []).append(rec)
    return sorted(groups.items(), key=lambda kv: kv[0])


def test_golden_set_has_a_group_of_two_or_more():
    assert any(len(recs) >= 2 for _, recs in golden_groups())


@pytest.fixture(scope="module")
def golden_scene(orc):
    return HostScene(orc)


@pytest.mark.parametrize("key,recs", golden_groups(), ids=[f"dof{k[0]}_{i}" for i, (k, _) in enumerate(golden_groups())])
def test_golden_group_as_one_batch(golden_scene, key, recs):
    dof = key[0]
    cfg = product_config(recs[0])
    cbs = [golden_scene.oracle_callbacks(dof, r["use_photo"], r["use_keypoints"]) for r in recs]
    rc, P, S, E, IT, ST, TR = capi.track_lm_batch(cfg, dof, batch_eval(cbs), [np.array(r["start_pose"], np.float32) for r in recs],
                                                  [r["start_scale"] for r in recs])
    assert rc == 0
    for b, rec in enumerate(recs):
        if rec["status"] == "no_overlap":
            assert ST[b] == SAGE_E_NO_OVERLAP and IT[b] == 0 and np.array_equal(P[b], np.array(rec["start_pose"], np.float32))
            continue
        assert ST[b] == 0 and IT[b] == rec["iters"]
        check_trace(TR[b], rec["trace"], 2e-5)
        assert float(E[b]) == pytest.approx(rec["final_error"], rel=2e-5)
        assert float(S[b]) == pytest.approx(rec["final_scale"], rel=1e-5)
        assert np.abs(P[b] - np.array(rec["final_pose"], np.float32)).max() < 2e-6
