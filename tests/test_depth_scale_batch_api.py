"""sage_depth_scale_ratio_batch, sage_median_f32_batch, their plan and launch count, and sage_loop_accept without a device:
the header declares them, the library exports them, the plan equals the formulas of include/sage_ba.h, every argument check
answers before anything touches the device, and sage_loop_accept's host rules on rounds in which nothing is accepted.  The
workspace handle of these calls is a zeroed block of host memory, as in tests/test_overlap_batch_api.py.

tests/loop_accept_ref.py (the restatement the GPU test compares with) is checked here against hand-derived cases.

The plan's formulas, for B >= 1 rows of M_b points (0 for B = 0):
  workgroups     sum_b min(ceil(M_b / 256), 256): the single call's partition per row, as one flat list
  device bytes   4 sum(M_b) + 24608 B: the keys, and per row 3 x 2048 bins, 4 counters, 2 x 2 words of pass state
  pinned bytes   32 B: a record per row
  launches       5: the per-point kernel, two digit passes, the finish, the ticket"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import loop_accept_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID = -1
NAMES = ("sage_depth_scale_ratio_batch", "sage_median_f32_batch", "sage_depth_scale_ratio_batch_plan",
         "sage_depth_scale_ratio_batch_launches", "sage_loop_accept")


def _fields(hdr, name):
    body = re.search(r"typedef struct " + name + r"[^{]*\{(.*?)\}\s*" + name + ";", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[\*\s]|\[\d+\]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return out


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"#define SAGE_DEPTH_SCALE_MAX_BATCH (\d+)", hdr).group(1) == str(capi.DEPTH_SCALE_MAX_BATCH) == "32"
    for name in ("SageDepthScaleRow", "SageLoopAcceptConfig", "SageLoopScaleQuery", "SageLoopScaleCandidate", "SageLoopInfo"):
        assert _fields(hdr, name) == [f[0] for f in getattr(capi, name)._fields_], name
    assert C.sizeof(capi.SageDepthScaleRow) == 48 + 3 * 8 + 8 + 2 * 8
    assert C.sizeof(capi.SageLoopInfo) == 8 + 8 + 48 + 16 + 24
    for f in (capi.depth_scale_ratio_batch, capi.median_f32_batch, capi.depth_scale_ratio_batch_plan, capi.loop_accept):
        assert callable(f)


# ---------------------------------------------------------------------------------------------------------------- the plan
MIXED = [1, 2, 255, 256, 257, 2176]


@pytest.mark.parametrize("M", [[2176], [2176] * 32, MIXED, [1] * 32, [58052] * 20, [1 << 20, 3]])
def test_plan_launches_five_whatever_the_rows(M):
    p = capi.depth_scale_ratio_batch_plan(M)
    assert p["launches"] == 5
    assert p["workgroups"] == sum(min(-(-m // 256), 256) for m in M)
    assert p["device_bytes"] == 4 * sum(M) + 24608 * len(M) and p["pinned_bytes"] == 32 * len(M)


def test_plan_of_an_empty_batch():
    assert capi.depth_scale_ratio_batch_plan([]) == dict(device_bytes=0, pinned_bytes=0, launches=0, workgroups=0)


def test_plan_bytes_grow_with_the_points():
    for B in (1, 4, 32):
        last = 0
        for m in (1, 2, 255, 256, 257, 2176, 58052):
            p = capi.depth_scale_ratio_batch_plan([m] * B)
            assert p["device_bytes"] > last and p["device_bytes"] >= 4 * m * B
            last = p["device_bytes"]
    a, b = capi.depth_scale_ratio_batch_plan([100, 5000]), capi.depth_scale_ratio_batch_plan([5000, 101])
    assert b["device_bytes"] == a["device_bytes"] + 4


def test_plan_checks_its_arguments_and_takes_null_outputs():
    raw = capi.depth_scale_ratio_batch_plan_raw
    M = (C.c_int32 * 33)(*([2176] * 33))
    assert raw(C.addressof(M), 3, None, None, None, None) == 0
    assert raw(None, 0, None, None, None, None) == 0 and raw(C.addressof(M), 0, None, None, None, None) == 0
    launches = C.c_int32(77)
    assert raw(C.addressof(M), 32, None, None, C.addressof(launches), None) == 0 and launches.value == 5
    bad_row = (C.c_int32 * 3)(5, 0, 5)
    neg_row = (C.c_int32 * 3)(5, 5, -1)
    for Mp, B in ((C.addressof(M), -1), (C.addressof(M), 33), (None, 1), (C.addressof(bad_row), 3), (C.addressof(neg_row), 3)):
        launches.value = 77
        assert raw(Mp, B, None, None, C.addressof(launches), None) == SAGE_E_INVALID and launches.value == 77
    assert raw(C.addressof(bad_row), 1, None, None, None, None) == 0          # (the bad row is not part of the batch)


# ---------------------------------------------------------------------------------------------- the batch's argument checks
class Args:
    """a valid argument set (B = 3) whose pointers are never followed: every case below changes one thing"""

    def __init__(self):
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        self.p = C.addressof(self.dummy)
        self.rows = (capi.SageDepthScaleRow * 33)()
        for r in self.rows:
            r.dpt0_dev, r.homo0_dev, r.M = self.p, self.p, 100
        self.cam = capi.SageCamera(57.6, 57.6, 31.5, 23.5, 64.0, 48.0)
        self.out = (capi.SageDepthScaleStats * 33)()
        for o in self.out:
            o.n_points = 77

    def batch(self, **kw):
        for k, v in kw.pop("cam_fields", {}).items():
            setattr(self.cam, k, v)
        for b, change in kw.pop("row_fields", {}).items():
            for k, v in change.items():
                setattr(self.rows[b], k, v)
        a = dict(ws=C.addressof(self.ws), rows=C.addressof(self.rows), B=3, cam=C.addressof(self.cam), bias1=self.p, mask=self.p,
                 out=C.addressof(self.out))
        a.update(kw)
        return capi.depth_scale_ratio_batch_raw(a["ws"], a["rows"], a["B"], a["cam"], a["bias1"], a["mask"], 1e-4, 1, a["out"])

    def untouched(self):
        return all(o.n_points == 77 for o in self.out)


INVALID = [dict(ws=None), dict(rows=None), dict(cam=None), dict(bias1=None), dict(mask=None), dict(out=None), dict(B=-1), dict(B=33),
           dict(row_fields={0: dict(M=0)}), dict(row_fields={2: dict(M=-4)}), dict(row_fields={1: dict(dpt0_dev=None)}),
           dict(row_fields={2: dict(homo0_dev=None)}), dict(cam_fields=dict(fx=0.0)), dict(cam_fields=dict(fy=-1.0)),
           dict(cam_fields=dict(fx=float("nan"))), dict(cam_fields=dict(fy=float("inf"))), dict(cam_fields=dict(w=0.5)),
           dict(cam_fields=dict(h=0.0)), dict(cam_fields=dict(w=float("nan")))]


@pytest.mark.parametrize("change", INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_batch_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.batch(**change) == SAGE_E_INVALID
    assert a.untouched()


def test_a_null_workspace_is_refused_first():
    a = Args()
    assert a.batch(ws=None, rows=None, cam=None, bias1=None, mask=None, out=None, B=99) == SAGE_E_INVALID
    n_kept = C.c_int32(77)
    assert capi.loop_accept_raw(None, None, None, None, None, None, None, 99, None, None, C.addressof(n_kept)) == SAGE_E_INVALID
    assert n_kept.value == 77
    assert capi.median_f32_batch_raw(None, None, None, None, 99, 0, None, None, None) == SAGE_E_INVALID


def test_an_empty_batch_launches_nothing_and_needs_no_device():
    a = Args()
    assert a.batch(B=0) == 0 and a.untouched()
    assert a.batch(B=0, row_fields={0: dict(M=0)}) == 0 and a.untouched()     # (no row is read)
    f = capi.lib().sage_depth_scale_ratio_batch_launches
    f.argtypes = [C.c_void_p]
    assert f(None) == 0 and f(C.addressof(a.ws)) == 0
    assert capi.depth_scale_ratio_batch_launches(None) == 0


def test_median_batch_refuses_invalid_arguments_without_a_device():
    ws = C.create_string_buffer(8192)
    dummy = C.create_string_buffer(64)
    vals = (C.c_void_p * 33)(*([C.addressof(dummy)] * 33))
    n = (C.c_int32 * 33)(*([10] * 33))
    med = (C.c_float * 33)(*([77.0] * 33))
    raw = capi.median_f32_batch_raw
    w, v, nn, m = C.addressof(ws), C.addressof(vals), C.addressof(n), C.addressof(med)
    assert raw(w, v, None, nn, 0, 0, m, None, None) == 0
    assert raw(w, None, None, None, 0, 0, None, None, None) == 0
    for args in ((None, v, None, nn, 3, 0, m), (w, None, None, nn, 3, 0, m), (w, v, None, None, 3, 0, m), (w, v, None, nn, 3, 0, None),
                 (w, v, None, nn, -1, 0, m), (w, v, None, nn, 33, 0, m)):
        assert raw(*args, None, None) == SAGE_E_INVALID, args
    n[1] = 0
    assert raw(w, v, None, nn, 3, 0, m, None, None) == SAGE_E_INVALID
    n[1] = 10
    vals[2] = None
    assert raw(w, v, None, nn, 3, 0, m, None, None) == SAGE_E_INVALID
    assert all(x == 77.0 for x in med)


# ------------------------------------------------------------------------------------------------- sage_loop_accept, host
CFG = dict(min_area_ratio=0.5, min_inlier_ratio=0.5, base_metric=0.3, base_desc_ratio=0.2, redundant_range=5, dpt_eps=1e-4)
GOOD = dict(tracked=1, status=0, area_ratio=0.8, inlier_ratio=0.7, area_inlier_ratio=0.56, desc=0.4)
NAN = float("nan")


class Round:
    """B candidates from dicts of the fields of tests/loop_accept_ref.py; their device pointers are a host dummy"""

    def __init__(self, cands, cfg=CFG):
        B = self.B = len(cands)
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        p = C.addressof(self.dummy)
        self.cfg = capi.SageLoopAcceptConfig(*[cfg[k] for k, _ in capi.SageLoopAcceptConfig._fields_])
        self.query = capi.SageLoopScaleQuery(p, p, capi.SageCamera(57.6, 57.6, 31.5, 23.5, 64.0, 48.0))
        self.cands = (capi.SageLoopCandidate * max(B, 1))()
        self.scands = (capi.SageLoopScaleCandidate * max(B, 1))()
        self.pre = (capi.SageLoopPrecheckResult * max(B, 1))()
        self.ver = (capi.SageLoopVerifyResult * max(B, 1))()
        for b, c in enumerate(cands):
            self.cands[b].dpt_map_dev = p
            self.scands[b] = capi.SageLoopScaleCandidate(c.get("id", b), p, p, 100, c.get("dpt_scale", 1.0), c.get("tracker_ref_scale", 1.0))
            self.pre[b].desc_match_inlier_ratio = c["desc"]
            v = self.ver[b]
            v.tracked, v.status, v.area_ratio, v.inlier_ratio, v.area_inlier_ratio = (c[k] for k in ("tracked", "status", "area_ratio",
                                                                                                      "inlier_ratio", "area_inlier_ratio"))
        self.infos = (capi.SageLoopInfo * max(B, 1))()
        self.kept = (C.c_int32 * max(B, 1))(*([77] * max(B, 1)))
        self.n_kept = C.c_int32(77)

    def call(self, **kw):
        a = dict(ws=C.addressof(self.ws), cfg=C.addressof(self.cfg), query=C.addressof(self.query), cands=C.addressof(self.cands),
                 scands=C.addressof(self.scands), pre=C.addressof(self.pre), ver=C.addressof(self.ver), B=self.B,
                 infos=C.addressof(self.infos), kept=C.addressof(self.kept), n_kept=C.addressof(self.n_kept))
        a.update(kw)
        return capi.loop_accept_raw(a["ws"], a["cfg"], a["query"], a["cands"], a["scands"], a["pre"], a["ver"], a["B"], a["infos"],
                                    a["kept"], a["n_kept"])


REJECTED = [dict(tracked=0), dict(status=-3), dict(status=1), dict(area_ratio=0.49), dict(inlier_ratio=0.2), dict(area_inlier_ratio=0.29),
            dict(desc=0.19), dict(area_ratio=NAN), dict(inlier_ratio=NAN), dict(area_inlier_ratio=NAN), dict(desc=NAN)]


def test_nothing_accepted_is_ok_and_launches_nothing():
    """every way to fail the accept test, NaNs included, side by side: SAGE_OK, n_kept = 0, every info zeroed -- on a workspace
    that is no workspace, so a launch would fault"""
    cands = [{**GOOD, **change} for change in REJECTED]
    assert not any(lref.accepted(CFG, c) for c in cands) and lref.accepted(CFG, GOOD)
    r = Round(cands)
    assert r.call() == 0
    assert r.n_kept.value == 0 and all(k == -1 for k in r.kept)
    assert bytes(memoryview(r.infos)) == bytes(C.sizeof(r.infos))
    assert lref.filter_kept(CFG, cands) == ([False] * len(cands), [])
    empty = Round([])
    assert empty.call() == 0 and empty.n_kept.value == 0
    assert empty.call(cands=None, scands=None, pre=None, ver=None) == 0


def test_the_accept_test_is_inclusive_at_its_thresholds():
    at = {**GOOD, "area_ratio": 0.5, "inlier_ratio": 0.5, "area_inlier_ratio": np.float32(0.3), "desc": np.float32(0.2)}
    assert lref.accepted(CFG, at)
    # the library agrees: such a candidate is accepted, which shows as the refusal of its NULL depth map (before any launch)
    r = Round([at])
    r.cands[0].dpt_map_dev = None
    assert r.call() == SAGE_E_INVALID and r.n_kept.value == 77


@pytest.mark.parametrize("change", [dict(ws=None), dict(cfg=None), dict(query=None), dict(infos=None), dict(kept=None), dict(n_kept=None),
                                    dict(B=-1), dict(B=33), dict(cands=None), dict(scands=None), dict(pre=None), dict(ver=None)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_loop_accept_refuses_invalid_arguments_without_a_device(change):
    r = Round([{**GOOD, "tracked": 0}] * 3)
    assert r.call(**change) == SAGE_E_INVALID
    assert r.n_kept.value == 77 and all(k == 77 for k in r.kept)


def _accepted_with(field, value, where):
    r = Round([{**GOOD, "tracked": 0}, dict(GOOD)])
    if where == "cands":
        setattr(r.cands[1], field, value)
    elif where == "scands":
        setattr(r.scands[1], field, value)
    elif where == "cam":
        setattr(r.query.cam, field, value)
    else:
        setattr(r.query, field, value)
    return r


@pytest.mark.parametrize("where,field,value", [
    ("cands", "dpt_map_dev", None), ("scands", "valid_loc1d_dev", None), ("scands", "valid_homo_dev", None), ("scands", "M", 0),
    ("scands", "dpt_scale", 0.0), ("scands", "dpt_scale", -1.0), ("scands", "dpt_scale", NAN), ("scands", "dpt_scale", float("inf")),
    ("scands", "tracker_ref_scale", 0.0), ("scands", "tracker_ref_scale", NAN), ("scands", "tracker_ref_scale", float("inf")),
    ("query", "bias_dev", None), ("query", "video_mask_dev", None), ("cam", "fx", 0.0), ("cam", "fy", NAN), ("cam", "w", 0.5)])
def test_loop_accept_refuses_a_bad_member_of_an_accepted_candidate_only(where, field, value):
    r = _accepted_with(field, value, where)
    assert r.call() == SAGE_E_INVALID and r.n_kept.value == 77
    # the same member on a candidate that is not accepted is not read
    r = _accepted_with(field, value, where)
    r.ver[1].tracked = 0
    assert r.call() == 0 and r.n_kept.value == 0


# --------------------------------------------------------------------------------- the restatement, on hand-derived cases
def _c(id, desc, **kw):
    return {**GOOD, "id": id, "desc": desc, **kw}


def test_ref_sort_keeps_candidate_order_on_a_tie():
    cands = [_c(100, 0.4), _c(200, 0.6), _c(300, 0.6), _c(400, 0.4)]
    assert lref.filter_kept(CFG, cands) == ([True] * 4, [1, 2, 0, 3])


def test_ref_redundant_range_is_exclusive():
    near = [_c(100, 0.4), _c(104, 0.6)]                 # |100 - 104| = 4 < 5: the lower-ranked one goes
    assert lref.filter_kept(CFG, near)[1] == [1]
    at = [_c(100, 0.4), _c(105, 0.6)]                   # |100 - 105| = 5 is not < 5: both stay
    assert lref.filter_kept(CFG, at)[1] == [1, 0]
    chain = [_c(100, 0.9), _c(104, 0.8), _c(108, 0.7)]  # 104 goes because of 100; 108 is 8 from 100 and is compared with kept ones only
    assert lref.filter_kept(CFG, chain)[1] == [0, 2]


def test_ref_first_ranked_is_always_kept():
    cands = [_c(7, 0.3), _c(7, 0.9), _c(7, 0.5)]
    assert lref.filter_kept(CFG, cands)[1] == [1]
    assert lref.filter_kept({**CFG, "redundant_range": 0}, cands)[1] == [1, 2, 0]
    mixed = [_c(7, 0.3, tracked=0), _c(8, 0.25), _c(9, 0.9, status=-3)]
    assert lref.filter_kept(CFG, mixed) == ([False, True, False], [1])


def test_ref_pose_of_a_quarter_turn():
    """R = a quarter turn about z (x -> y), t = (1, 2, 3): R^T t = (2, -1, 3), so t_cur_ref = -(2, -1, 3) * 3 / 2 = (-3, 1.5, -4.5),
    every step exact in fp32"""
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    pose12 = np.concatenate([R.reshape(9), np.array([1, 2, 3], np.float32)])
    Rt, t = lref.pose(pose12, 3.0, 2.0)
    assert Rt.dtype == np.float32 and t.dtype == np.float32
    assert np.array_equal(Rt, R.T) and np.array_equal(t, np.array([-3.0, 1.5, -4.5], np.float32))
    assert np.array_equal(Rt @ R, np.eye(3, dtype=np.float32))


def test_ref_pose_rounds_once_per_operation():
    rng = np.random.default_rng(11)
    p = rng.standard_normal(12).astype(np.float32)
    Rt, t = lref.pose(p, 1.3, 0.7)
    R, tt = p[:9].reshape(3, 3).astype(np.float64), p[9:].astype(np.float64)
    want = -(R.T @ tt) * np.float64(np.float32(1.3)) / np.float64(np.float32(0.7))
    assert np.allclose(t, want, rtol=4 * 2.0 ** -23, atol=4 * 2.0 ** -23 * np.abs(R.T * tt).sum(1).max() * 2)
