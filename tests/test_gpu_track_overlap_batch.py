"""sage_track_overlap_batch on the device: B poses over one point set, camera and mask in three launches and one wait.

The contract is BYTE-EQUALITY with the single call: row b of a batch equals sage_track_overlap with poses[b], the whole
SageOverlapStats, n_candidates included -- a row keeps the single call's partition (min(ceil(M / 256), 32) workgroups), its
device functions and its sums in workgroup order.  The single calls run on a workspace of their own and on the batch's.

Shapes (synth.make_overlap_problem, seed 1; poses synth.OVERLAP_POSES): 48x64 (M = 2176: 9 workgroups per row), 96x128
(M = 8708: more points than the 32 workgroups of one grid pass hold), and slices of 1, 2, 255, 256 and 257 points from the
middle of the 48x64 image (one lane, one workgroup to the brim, a second workgroup of one lane).  B = 1, 2, 3, 32.

Equality with a single call that is itself wrong would prove nothing: one batch of the three poses is compared with the
fp64 restatement of tests/overlap_ref.py under the rule of tests/test_gpu_track_overlap.py -- a quantity may be off by 8 x
the larger of the fp32 restatement's own relative distance from fp64 (computed here, on the CPU) and 2^-24; the counts are
exact up to the ambiguous points, of which there are at most 0.005 M."""
import ctypes as C
import functools

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import edge_scenes as es
from tests import overlap_ref as ref

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
POSES = ("small", "big", "behind")


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


@pytest.fixture(scope="module")
def ws_single(capi):
    """the single calls' own workspace"""
    w = capi.Workspace()
    yield w
    w.close()


def pose_of(name):
    rot, tr = synth.OVERLAP_POSES[name]
    return synth.so3_exp(np.asarray(rot, np.float64)).astype(np.float32), np.asarray(tr, np.float32)


@functools.lru_cache(maxsize=None)
def problem(H, W, M=None):
    """the point set of seed 1 (whole, or M points from the middle of the image) and its device arrays: made once"""
    import torch
    prob = synth.make_overlap_problem(H, W, seed=1)
    if M is not None:
        mid = prob["M"] // 2
        prob = {**prob, "dpts0": prob["dpts0"][mid:mid + M], "homo": prob["homo"][mid:mid + M], "M": M}
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return prob, dict(dpts0=dv(prob["dpts0"]), homo=dv(prob["homo"]), mask=dv(prob["mask"]), zero_mask=dv(np.zeros_like(prob["mask"])))


def rows_of(names, scales=None):
    return [(*pose_of(n), 1.0 if scales is None else scales[i]) for i, n in enumerate(names)]


def batch(capi, ws, pd, rows, eps=None, mask="mask"):
    prob, dev = pd
    return capi.track_overlap_batch(ws, rows, dev["dpts0"], dev["homo"], prob["cam"], dev[mask], prob["eps"] if eps is None else eps)


def single(capi, ws, pd, row, eps=None, mask="mask"):
    prob, dev = pd
    R, t, ds = row
    return capi.track_overlap(ws, R, t, dev["dpts0"], dev["homo"], prob["cam"], dev[mask], prob["eps"] if eps is None else eps, ds)


def raw(st):
    return bytes(memoryview(st))


def assert_rows_are_the_single_calls(capi, ws, ws_single, pd, rows, **kw):
    own = [raw(single(capi, ws_single, pd, r, **kw)) for r in rows]
    got = [raw(st) for st in batch(capi, ws, pd, rows, **kw)]
    same_ws = [raw(single(capi, ws, pd, r, **kw)) for r in rows]
    again = [raw(st) for st in batch(capi, ws, pd, rows, **kw)]       # (after single calls have used the regions in between)
    assert len(got) == len(rows)
    for b in range(len(rows)):
        assert got[b] == own[b], f"row {b}: batch != single call on a workspace of its own"
        assert got[b] == same_ws[b], f"row {b}: batch != single call on the batch's workspace"
        assert again[b] == got[b], f"row {b}: second batch"
    return got


# ---- 1. row b equals the single call
ORDERS = {"small-big-behind": POSES, "behind-big-small": POSES[::-1], "small": POSES[:1], "big": POSES[1:2], "behind": POSES[2:]}


@pytest.mark.parametrize("order", list(ORDERS))
def test_rows_equal_the_single_calls_byte_for_byte(capi, ws, ws_single, order):
    pd = problem(48, 64)
    assert pd[0]["M"] == 2176 and capi.track_overlap_batch_plan(2176, 3)["workgroups_per_row"] == 9
    got = assert_rows_are_the_single_calls(capi, ws, ws_single, pd, rows_of(ORDERS[order]))
    assert len(set(got)) == len(got)                                     # (the poses do give different rows)


def test_thirty_two_rows_of_different_depth_scales(capi, ws, ws_single):
    rows = rows_of([POSES[b % 3] for b in range(32)], [1.0 + 0.01 * b for b in range(32)])
    got = assert_rows_are_the_single_calls(capi, ws, ws_single, problem(48, 64), rows)
    assert len(set(got)) == 32


def test_more_points_than_one_grid_pass(capi, ws, ws_single):
    pd = problem(96, 128)
    assert pd[0]["M"] == 8708 and capi.track_overlap_batch_plan(8708, 3)["workgroups_per_row"] == 32
    assert_rows_are_the_single_calls(capi, ws, ws_single, pd, rows_of(POSES))


@pytest.mark.parametrize("M", [1, 2, 255, 256, 257])
def test_few_points_and_the_workgroup_boundary(capi, ws, ws_single, M):
    pd = problem(48, 64, M)
    got = assert_rows_are_the_single_calls(capi, ws, ws_single, pd, rows_of(["small", "big"]))
    st = batch(capi, ws, pd, rows_of(["small", "big"]))
    assert [s.n_points for s in st] == [M, M] and st[0].n_pos_depth == M and got[0] != got[1]


# ---- 2. against the fp64 restatement
def bound(v32, v64):
    """8 x the larger of the fp32 restatement's relative distance from the fp64 one and 2^-24"""
    return 8.0 * max(abs(v32 - v64) / abs(v64), EPS24)


def close(got, want, rel, what):
    d = abs(got - want) / abs(want)
    print(f"    {what}: got {got!r} want {want!r} rel {d:.2e} bound {rel:.2e}")
    return d <= rel


@functools.lru_cache(maxsize=None)
def restated(name):
    """(fp64 statistics, fp32 statistics, ambiguous points) of the 48x64 point set under the named pose"""
    R, t = pose_of(name)
    prob = {**problem(48, 64)[0], "R": R, "t": t}
    return ref.stats(prob, np.float64), ref.stats(prob, np.float32), int(ref.ambiguous(prob).sum())


def test_one_batch_of_the_three_poses_matches_the_fp64_restatement(capi, ws):
    pd = problem(48, 64)
    M = pd[0]["M"]
    for name, st in zip(POSES, batch(capi, ws, pd, rows_of(POSES))):
        s64, s32, n_amb = restated(name)
        print(f"{name}: M {M} ambiguous {n_amb}  pos {st.n_pos_depth}/{s64['n_pos_depth']}  in {st.n_in_mask}/{s64['n_in_mask']}  "
              f"candidates {list(st.n_candidates)}")
        assert st.n_points == M
        assert n_amb <= 0.005 * M
        assert abs(st.n_pos_depth - s64["n_pos_depth"]) <= n_amb and abs(st.n_in_mask - s64["n_in_mask"]) <= n_amb
        assert st.inlier_ratio == np.float32(st.n_in_mask) / np.float32(M)
        assert close(st.input_area, s64["input_area"], bound(s32["input_area"], s64["input_area"]), "input_area")
        assert 0 < st.n_candidates[0] <= M
        if s64["n_in_mask"] == 0:
            assert name == "behind" and 0 < s64["n_pos_depth"] < M
            assert st.n_in_mask == 0 and st.warp_area == 0.0 and st.area_ratio == 0.0 and st.n_candidates[1] == 0
        else:
            assert close(st.warp_area, s64["warp_area"], bound(s32["warp_area"], s64["warp_area"]), "warp_area")
            assert close(st.area_ratio, s64["area_ratio"], bound(s32["area_ratio"], s64["area_ratio"]), "area_ratio")
            assert 0 < st.n_candidates[1] <= st.n_in_mask
        assert close(st.average_motion, s64["average_motion"], bound(s32["average_motion"], s64["average_motion"]), "average_motion")
    assert restated("behind")[0]["n_in_mask"] == 0 and restated("small")[0]["n_in_mask"] > 0 and restated("big")[0]["n_in_mask"] > 0


# ---- 3. an empty set does not leak
def test_an_empty_row_on_either_side_leaves_its_neighbour_alone(capi, ws, ws_single):
    pd = problem(48, 64)
    M = pd[0]["M"]
    rows = rows_of(["behind", "small", "behind"])
    st = batch(capi, ws, pd, rows)
    b64, _, b_amb = restated("behind")
    s64, _, s_amb = restated("small")
    assert b64["n_in_mask"] == 0
    for k in (0, 2):
        assert abs(st[k].n_pos_depth - b64["n_pos_depth"]) <= b_amb and 0 < st[k].n_pos_depth < M
        assert st[k].n_in_mask == 0 and st[k].warp_area == 0.0 and st[k].n_candidates[1] == 0 and st[k].area_ratio == 0.0
        assert np.isfinite(st[k].average_motion)
    assert raw(st[0]) == raw(st[2])
    assert abs(st[1].n_pos_depth - s64["n_pos_depth"]) <= s_amb and abs(st[1].n_in_mask - s64["n_in_mask"]) <= s_amb
    assert st[1].warp_area > 0.0 and st[1].n_candidates[1] >= 3
    assert raw(st[1]) == raw(single(capi, ws_single, pd, rows[1]))


def test_a_batch_whose_only_set_is_empty(capi, ws, ws_single):
    pd = problem(48, 64)
    s64, s32, s_amb = restated("small")
    rows = rows_of(["small"])
    (st,) = batch(capi, ws, pd, rows, eps=np.float32(1e6))               # no depth passes: nothing is positive
    assert st.n_pos_depth == 0 and st.n_in_mask == 0 and st.warp_area == 0.0 and st.n_candidates[1] == 0
    assert np.isnan(st.average_motion) and st.area_ratio == 0.0
    assert close(st.input_area, s64["input_area"], bound(s32["input_area"], s64["input_area"]), "input_area")
    assert raw(st) == raw(single(capi, ws_single, pd, rows[0], eps=np.float32(1e6)))
    (st,) = batch(capi, ws, pd, rows, mask="zero_mask")                  # the mask lets nothing in
    assert abs(st.n_pos_depth - s64["n_pos_depth"]) <= s_amb and st.n_pos_depth > 0
    assert st.n_in_mask == 0 and st.warp_area == 0.0 and st.n_candidates[1] == 0 and st.inlier_ratio == 0.0
    assert np.isfinite(st.average_motion) and st.average_motion > 0
    assert raw(st) == raw(single(capi, ws_single, pd, rows[0], mask="zero_mask"))
    (st,) = batch(capi, ws, pd, rows)                                    # ... and nothing of either stays behind
    assert raw(st) == raw(single(capi, ws_single, pd, rows[0])) and st.n_candidates[1] > 0


# ---- 4. the input set is done once
def test_every_row_carries_the_one_input_set(capi, ws, ws_single):
    pd = problem(48, 64)
    rows = rows_of([POSES[b % 3] for b in range(7)], [1.0 + 0.05 * b for b in range(7)])
    st = batch(capi, ws, pd, rows)
    one = single(capi, ws_single, pd, rows[2])
    for s in st:
        assert s.input_area == one.input_area and s.n_candidates[0] == one.n_candidates[0]
    assert 0 < one.n_candidates[0] < pd[0]["M"]


def test_a_set_that_is_all_hull_survives_whole_in_every_row(capi, ws):
    """the circle of tests/test_gpu_track_overlap.py (360 source pixels, every one a hull vertex) under four small
    translations: no row drops a point of the input set, and every row's warped set -- the same circle, shifted -- stays whole"""
    import torch
    cam = synth.Camera(*[np.float32(v) for v in (288.0, 288.0, 159.5, 127.5, 320.0, 256.0)])
    a = 2.0 * np.pi * np.arange(360) / 360
    x, y = 159.5 + 100.0 * np.cos(a), 127.5 + 100.0 * np.sin(a)
    homo = np.stack([(x - 159.5) / 288.0, (y - 127.5) / 288.0, np.ones(360)], 1).astype(np.float32)
    prob = dict(cam=cam, mask=np.ones((256, 320), np.float32), dpts0=np.ones(360, np.float32), homo=homo, eps=np.float32(1e-4), M=360)
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    pd = (prob, dict(dpts0=dv(prob["dpts0"]), homo=dv(homo), mask=dv(prob["mask"])))
    eye = np.eye(3, dtype=np.float32)
    rows = [(eye, np.array(t, np.float32), 1.0) for t in ((0, 0, 0), (0.01, 0, 0), (0, -0.02, 0), (0.015, 0.01, 0))]
    st = batch(capi, ws, pd, rows)
    p32 = ref.points({**prob, "R": eye, "t": np.zeros(3, np.float32)}, np.float32)
    want, corners = ref.hull(np.stack([p32["x0"], p32["y0"]], 1))
    assert len(corners) == 360
    for s in st:
        assert s.n_candidates[0] == 360 and s.n_in_mask == s.n_pos_depth == 360 and s.n_candidates[1] == 360
        assert close(s.input_area, want, 8 * EPS24, "input_area vs fp64 hull of the fp32 points")
        assert close(s.warp_area, want, 1e-6, "warp_area")
    assert st[0].average_motion < 1e-6 < st[1].average_motion


# ---- 5. determinism
def test_identical_rows_and_repeated_calls_give_identical_bytes(capi, ws):
    pd = problem(96, 128)
    rows = rows_of(["big", "small", "big", "big"])
    a = [raw(s) for s in batch(capi, ws, pd, rows)]
    b = [raw(s) for s in batch(capi, ws, pd, rows)]
    assert a[0] == a[2] == a[3] != a[1]
    assert a == b
    w2 = capi.Workspace()                                                # a fresh workspace (fresh buffers) too
    try:
        assert [raw(s) for s in batch(capi, w2, pd, rows)] == a
    finally:
        w2.close()


# ---- 6. launches
def test_three_launches_whatever_B(capi):
    pd = problem(48, 64)
    prob, dev = pd
    w = capi.Workspace()
    try:
        assert capi.track_overlap_batch_launches(w) == 0                 # none yet
        for B in (1, 3, 32):
            assert len(batch(capi, w, pd, rows_of([POSES[b % 3] for b in range(B)]))) == B
            assert capi.track_overlap_batch_launches(w) == 3 == capi.track_overlap_batch_plan(prob["M"], B)["launches"]
        out = (capi.SageOverlapStats * 2)()
        C.memset(C.addressof(out), 0x5A, C.sizeof(out))
        before = bytes(out)
        cam = capi.SageCamera(*[float(v) for v in (prob["cam"].fx, prob["cam"].fy, prob["cam"].cx, prob["cam"].cy, prob["cam"].w, prob["cam"].h)])
        poses = (capi.SageOverlapPose * 1)()
        assert capi.track_overlap_batch_raw(w.h, C.addressof(poses), 0, capi.dptr(dev["dpts0"]), capi.dptr(dev["homo"]), prob["M"],
                                            C.addressof(cam), capi.dptr(dev["mask"]), 1e-4, C.addressof(out)) == 0
        assert bytes(out) == before and capi.track_overlap_batch_launches(w) == 0
        assert batch(capi, w, pd, []) == []
    finally:
        w.close()


# ---- 7. one workspace shared with the single call
def test_the_single_call_around_a_batch_that_grows_the_regions(capi):
    small, big = problem(48, 64), problem(96, 128)
    row = rows_of(["small"])[0]
    w = capi.Workspace()
    try:
        first = raw(single(capi, w, small, row))
        rows = rows_of([POSES[b % 3] for b in range(32)], [1.0 + 0.01 * b for b in range(32)])
        st = batch(capi, w, big, rows)
        assert len(st) == 32 and st[0].n_points == 8708
        plan = capi.track_overlap_batch_plan(8708, 32)
        assert plan["pinned_bytes"] > capi.track_overlap_batch_plan(2176, 1)["pinned_bytes"]
        third = raw(single(capi, w, small, row))
        assert first == third
        assert raw(st[5]) == raw(single(capi, w, big, rows[5]))
    finally:
        w.close()


# ---- 8. sage_loop_verify goes through the batch
CYC_THRESH, MULT, MG_WEIGHT, DIVISOR = 1.0, 2.0, 3.0, 1.25


def test_loop_verify_takes_its_overlap_statistics_from_one_batch(capi, orc):
    """the fixture of tests/test_gpu_track_batch.py (32x40, C = 16, K = 64, B = 4: planted, self, unrelated, planted; the self
    candidate cut to three inliers) -- the overlap fields of every tracked result equal one sage_track_overlap_batch over
    the returned poses, and the workspace's last batch spent three launches"""
    import torch
    from tests.test_gpu_tracker import Scene
    F = np.float32
    s = Scene(capi, orc, **es.LM_SCENE)
    ws = s.ws
    try:
        sc = synth.make_loop_candidates(3, 4, H=32, W=40, C=16, K=64, grid=2)
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        B, K, cam = 4, sc["K"], sc["cam"]
        cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
        arr = (capi.SageLoopCandidate * B)(*[capi.SageLoopCandidate(*[capi.dptr(c[n]).value for n in ("desc", "dpt_map", "kp_loc",
                                                                                                    "kp_dpts0", "kp_homo0")]) for c in cands])
        ccam = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
        prm = capi.registration_params(synth.registration_params(1.0))
        pre = (capi.SageLoopPrecheckResult * B)()
        rawm = torch.zeros(B, K, dtype=torch.int64, device="cuda")
        flags = torch.zeros(B, K, dtype=torch.int32, device="cuda")
        ikp = torch.zeros(B, K, dtype=torch.int32, device="cuda")
        desc_q = cu(sc["desc_q"])
        assert capi.loop_precheck_raw(ws.h, capi.dptr(desc_q), DIVISOR, C.addressof(arr), B, K, 16, 32, 40, C.addressof(ccam), CYC_THRESH,
                                      MULT, 0.3, C.addressof(prm), C.addressof(pre), capi.dptr(rawm), capi.dptr(flags),
                                      capi.dptr(ikp)) == 0
        assert pre[2].registered == 0 and all(pre[b].registered == 1 and pre[b].reg.n_inliers > 3 for b in (0, 1, 3))
        pre[1].reg.n_inliers = 3
        q = capi.SageLoopVerifyQuery()
        q.N = s.a.homo.shape[0]; q.FS = s.w.FS
        q.homo_dev = s.dev["homo"].data_ptr(); q.unscaled_dpts0_dev = s.dev["unscaled"].data_ptr()
        q.feat0s_dev = s.dev["f0s"].data_ptr(); q.weights_dev = s.dev["wts"].data_ptr()
        q.pyr = capi.make_pyramid(cam, s.w.L); q.eps = s.w.eps
        vy, vx = np.nonzero(s.w.mask > 0.5)
        vhomo = cu(np.stack([(vx - cam.cx) / cam.fx, (vy - cam.cy) / cam.fy, np.ones(vx.size)], 1).astype(F))
        vd = cu((F(DIVISOR) * (s.a.bias + s.a.basis @ s.a.code_true)[vy * 40 + vx]).astype(F))
        q.M = vx.size; q.valid_homo_dev = vhomo.data_ptr(); q.valid_dpts0_dev = vd.data_ptr(); q.mask_dev = s.dev["mask"].data_ptr()
        vcands = [dict(feat1=s.dev["feat1"], grad1=s.dev["grad1"], mask1=s.dev["mask"], kp_loss_param=s.mg_loss_param * (1 + 0.1 * b))
                  for b in range(B)]
        cfg = capi.lm_config_default()
        assert capi.track_overlap_batch_launches(ws) == 0
        res, _ = capi.loop_verify(ws, cfg, q, DIVISOR, cands, vcands, pre, rawm, ikp, MG_WEIGHT)
        assert capi.track_overlap_batch_launches(ws) == 3                # the stage went through the batch
        tracked = [b for b in range(B) if res[b].tracked == 1 and res[b].status == 0]
        assert tracked == [0, 3]
        rows = [(np.array(res[b].pose12[:9], F), np.array(res[b].pose12[9:], F), float(F(res[b].scale) / F(DIVISOR))) for b in tracked]
        w2 = capi.Workspace()
        try:
            ov = capi.track_overlap_batch(w2, rows, vd, vhomo, cam, s.dev["mask"], q.eps)
        finally:
            w2.close()
        for b, o in zip(tracked, ov):
            r = res[b]
            for k in ("area_ratio", "inlier_ratio", "average_motion"):
                assert F(getattr(r, k)).tobytes() == F(getattr(o, k)).tobytes(), (b, k)
            assert F(r.area_inlier_ratio).tobytes() == (F(o.area_ratio) * F(o.inlier_ratio)).tobytes()
            assert o.n_points == q.M and o.n_pos_depth > 0
        for b in (1, 2):
            assert res[b].tracked == 0 and res[b].area_ratio == 0 and res[b].inlier_ratio == 0
    finally:
        s.close()
