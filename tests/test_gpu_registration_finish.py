"""The finish of a registration on the device (reg_finish_kernel: SAGE_REG_FINISH_DEVICE, sage_registration_finish_batch) against
the fp64 restatement of tests/registration_ref.py, the fixtures the reference's solver wrote, and the host finish.

Exact: the inlier list, the rotation mask, rotation_iterations and every count -- tests/test_registration_ref.py shows on the
CPU that every discrete margin of the fixtures (weights, cost_diff, mu, translation membership, cost gap) exceeds 1e-6.
R, t: registration_ref.rotation_bound / translation_bound, the project's bounds for two fp64 evaluations of the finish that
differ in summation order and SVD (translation_bound is fed the rotation BOUND, not the measured distance).  The whole solve
adds the vote's share: 8 x the change the restatement's finish shows when fed scale (1 +- the vote's bound), as
tests/test_gpu_registration.py.

The kernel's edges among the fixtures: N = 2 (antiparallel TIMs: the rotation about their direction is open, compared as in
test_gpu_registration.py) and 3; 33 (a partial wave) and 64 (one wave); 257 (lane 0 carries a second TIM); 1024 (the 2048
endpoints fill the LDS tile); noise_free (leaves at mu <= 0), all_outliers, clamp, coincident_*.

Measured on an MI355X: the finish alone at the restatement's scale, distance -> bound

  n2                   (R, t: open at N = 2)
  n3                   |dR| 4.86e-16 -> 1.20e-12   |dt| 1.94e-16 -> 3.16e-12
  n33                  |dR| 6.11e-16 -> 9.87e-11   |dt| 7.42e-16 -> 5.48e-10
  n64_o0               |dR| 4.44e-16 -> 1.32e-12   |dt| 5.72e-16 -> 7.76e-12
  n64_o30              |dR| 3.33e-16 -> 2.22e-09   |dt| 2.36e-16 -> 1.28e-08
  n64_o70              |dR| 7.77e-16 -> 1.03e-08   |dt| 7.77e-16 -> 4.40e-08
  n64_all_outliers     |dR| 3.11e-14 -> 2.76e-07   |dt| 4.73e-14 -> 2.13e-06
  n64_noise_free       |dR| 2.53e-16 -> 2.75e-12   |dt| 2.26e-16 -> 1.23e-11
  n64_coincident_dst   |dR| 5.55e-16 -> 1.12e-10   |dt| 3.47e-16 -> 5.75e-10
  n64_coincident_src   |dR| 5.55e-16 -> 7.21e-11   |dt| 7.91e-16 -> 4.43e-10
  n64_clamp            |dR| 1.11e-15 -> 2.72e-10   |dt| 2.71e-18 -> 2.15e-11
  n257                 |dR| 2.78e-16 -> 6.08e-10   |dt| 2.22e-16 -> 3.11e-09
  n512_o50             |dR| 5.55e-16 -> 2.23e-09   |dt| 2.93e-16 -> 9.77e-09
  n1024                |dR| 7.77e-16 -> 2.22e-09   |dt| 2.29e-16 -> 1.63e-08
"""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import registration_ref as ref

pytestmark = pytest.mark.gpu

ALL_CASES = list(ref.CASES)
INT_FIELDS = ("valid", "n_inliers", "n_pairs", "n_degenerate_pairs", "n_scale_inlier_pairs", "rotation_iterations", "n_rotation_inliers")


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    """a workspace in DEVICE mode"""
    w = capi.Workspace()
    w.set_registration_finish(capi.SAGE_REG_FINISH_DEVICE)
    yield w
    w.close()


@pytest.fixture(scope="module")
def ws_host(capi):
    """a workspace that never switched"""
    w = capi.Workspace()
    yield w
    w.close()


def _problem(name):
    import torch
    fx, params = ref.load_case(name)
    q = {k: torch.from_numpy(fx[k]).cuda() for k in ("src", "dst", "noise_bounds")}
    q["noise_bound"] = params["noise_bound"]
    return q, params


def _np(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in o.items()}


def _same_bytes(a, b, what):
    a, b = _np(a), _np(b)
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _n2_rotation_is_a_rotation_onto_the_dst_tim(fx, R):
    u_s = fx["src"][1].astype(np.float64) - fx["src"][0]; u_d = fx["dst"][1].astype(np.float64) - fx["dst"][0]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0
    assert np.allclose(R @ (u_s / np.linalg.norm(u_s)), u_d / np.linalg.norm(u_d), atol=1e-12)


# ---- 1. the finish alone
@pytest.mark.parametrize("name", ALL_CASES)
def test_finish_alone_equals_the_restatement(capi, ws_host, name):
    from tests.conftest import summary_line
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    n = fx["src"].shape[0]
    q, _ = _problem(name)
    d = capi.registration_finish_batch(ws_host, [q], [r["scale"]], params, device_inliers=True)[0]
    assert d["valid"] == 1 and np.float64(d["scale"]).tobytes() == np.float64(r["scale"]).tobytes()
    assert d["n_inliers"] == r["n_inliers"] and np.array_equal(d["inliers"], r["inliers"])
    assert np.array_equal(d["inliers_dev"].cpu().numpy(), r["inliers"])
    assert np.array_equal(d["rotation_mask"], r["rotation_mask"]) and d["n_rotation_inliers"] == r["n_rotation_inliers"]
    assert d["rotation_iterations"] == r["rotation_iterations"]
    assert d["n_pairs"] == 0 and d["n_scale_inlier_pairs"] == 0 and d["scale_cost"] == 0      # (the vote's fields)
    if bool(fx["reference"]):
        assert np.array_equal(d["inliers"], fx["ref_inliers"]) and d["n_rotation_inliers"] == int(fx["ref_rotation_mask"].sum())
    if n == 2:
        _n2_rotation_is_a_rotation_onto_the_dst_tim(fx, d["R"])
        summary_line(f"registration finish {name:20s} (R, t: open at N = 2)")
        return
    b_R = ref.rotation_bound(r, n); b_t = ref.translation_bound(r, n, b_R, 0.0)
    d_R = np.abs(d["R"] - r["R"]).max(); d_t = np.abs(d["t"] - r["t"]).max()
    summary_line(f"registration finish {name:20s} |dR| {d_R:.2e} -> {b_R:.2e}   |dt| {d_t:.2e} -> {b_t:.2e}")
    assert d_R <= b_R and d_t <= b_t


# ---- 2. the whole solve in DEVICE mode
@pytest.mark.parametrize("name", ALL_CASES)
def test_device_mode_solve_equals_the_fixture(capi, ws, name):
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    n = fx["src"].shape[0]
    q, _ = _problem(name)
    d = capi.robust_registration(ws, q["src"], q["dst"], q["noise_bounds"], params, device_inliers=True)
    exp_inliers = fx["ref_inliers"] if bool(fx["reference"]) else r["inliers"]
    exp_scale_pairs = int(fx["ref_n_scale_inlier_pairs"]) if bool(fx["reference"]) else r["n_scale_inlier_pairs"]
    exp_rot = int(fx["ref_rotation_mask"].sum()) if bool(fx["reference"]) else r["n_rotation_inliers"]
    assert d["valid"] == 1
    assert d["n_pairs"] == n * (n - 1) // 2 and d["n_degenerate_pairs"] == r["n_degenerate_pairs"]
    assert d["n_scale_inlier_pairs"] == exp_scale_pairs
    assert d["n_inliers"] == exp_inliers.size and np.array_equal(d["inliers"], exp_inliers)
    assert np.array_equal(d["inliers_dev"].cpu().numpy(), exp_inliers)
    assert d["n_rotation_inliers"] == exp_rot
    assert d["rotation_iterations"] == r["rotation_iterations"]
    b_s = r["bound"]
    assert abs(d["scale"] - r["scale"]) / abs(r["scale"]) <= b_s
    assert abs(d["scale_cost"] - r["scale_cost"]) <= 1e-9 * abs(r["scale_cost"]) + 1e-12
    if n == 2:
        _n2_rotation_is_a_rotation_onto_the_dst_tim(fx, d["R"])
        return
    ch_R = ch_t = 0.0
    for s in (r["scale"] * (1 + b_s), r["scale"] * (1 - b_s)):
        f = ref.finish(fx["src"], fx["dst"], fx["noise_bounds"], s, params)
        assert np.array_equal(f["inliers"], r["inliers"])
        ch_R = max(ch_R, np.abs(f["R"] - r["R"]).max()); ch_t = max(ch_t, np.abs(f["t"] - r["t"]).max())
    b_R = ref.rotation_bound(r, n); b_t = ref.translation_bound(r, n, b_R, 0.0)
    assert np.abs(d["R"] - r["R"]).max() <= 8 * ch_R + b_R and np.abs(d["t"] - r["t"]).max() <= 8 * ch_t + b_t


# ---- 3. the batch contract
BATCH_NAMES = ("n512_o50", "n257", "n64_o30", "n33", "n3", "n2")


def _mixed_batch():
    """the six fixture problems, then N = 1, N = 0 and a problem whose vote is empty (every src point coincident)"""
    import torch
    probs = [_problem(n)[0] for n in BATCH_NAMES]
    for N in (1, 0):
        # (views of two points: the single call wants its pointers whatever N)
        probs.append(dict(src=torch.zeros(2, 3, device="cuda")[:N], dst=torch.zeros(2, 3, device="cuda")[:N],
                          noise_bounds=torch.full((2,), 0.01, device="cuda")[:N], noise_bound=0.01))
    same = torch.full((5, 3), 0.25, device="cuda")
    probs.insert(3, dict(src=same, dst=torch.arange(15, dtype=torch.float32, device="cuda").reshape(5, 3).contiguous(),
                         noise_bounds=torch.full((5,), 0.01, device="cuda"), noise_bound=0.01))
    return probs


def test_batch_rows_equal_the_single_calls_in_device_mode(capi, ws):
    _, params = ref.load_case("n33")
    probs = _mixed_batch()
    Ns = [int(q["src"].shape[0]) for q in probs]
    assert Ns == [512, 257, 64, 5, 33, 3, 2, 1, 0]
    single = []
    for q in probs:
        p = dict(params, noise_bound=q["noise_bound"])
        if q["src"].shape[0] == 0:       # (an empty tensor has no pointer: the single call with N = 0 on another problem's arrays)
            res = capi.SageRegistrationResult()
            prm = capi.registration_params(p)
            assert capi.robust_registration_raw(ws.h, capi.dptr(probs[0]["src"]), capi.dptr(probs[0]["dst"]), capi.dptr(probs[0]["noise_bounds"]),
                                                0, C.addressof(prm), C.addressof(res), None, None) == 0
            o = capi._reg_result(res)
            o.update(inliers=np.zeros(0, np.int32), inliers_dev=np.zeros(0, np.int32))
            single.append(_np(o))
            continue
        single.append(_np(capi.robust_registration(ws, q["src"], q["dst"], q["noise_bounds"], p, device_inliers=True)))
    assert single[3]["valid"] == 0 and single[3]["n_pairs"] == 10 and single[3]["n_degenerate_pairs"] == 10 and single[3]["n_inliers"] == 0
    assert single[7]["valid"] == 0 and single[8]["valid"] == 0
    for b, name in zip((0, 1, 2, 4, 5, 6), BATCH_NAMES):
        assert single[b]["valid"] == 1 and np.array_equal(single[b]["inliers"], ref.restated(name)["inliers"]), name
    for order in (list(range(len(probs))), list(range(len(probs)))[::-1]):
        batch = [probs[b] for b in order]
        first = capi.robust_registration_batch(ws, batch, params, device_inliers=True)
        assert capi.robust_registration_batch_launches(ws) == capi.registration_finish_plan([Ns[b] for b in order])["launches"]
        again = capi.robust_registration_batch(ws, batch, params, device_inliers=True)
        for row, b in enumerate(order):
            _same_bytes(first[row], single[b], (order[0], b))
            _same_bytes(again[row], single[b], (order[0], b, "again"))
    # the plan also names what the host-mode plan does not: the finish's launch
    host_plan = capi.robust_registration_batch_plan(Ns)
    assert capi.registration_finish_plan(Ns)["launches"] == host_plan["launches"] + 1
    # nothing votes: nothing is launched
    none = capi.robust_registration_batch(ws, [probs[7], probs[8], probs[7]], params, device_inliers=True)
    assert all(o["valid"] == 0 and o["n_inliers"] == 0 for o in none) and capi.robust_registration_batch_launches(ws) == 0
    # one voting problem among rows that do not vote: the single call's launches + 1
    one = capi.robust_registration_batch(ws, [probs[7], probs[4], probs[8]], params, device_inliers=True)
    _same_bytes(one[1], single[4], "one voting row")
    assert capi.robust_registration_batch_launches(ws) == capi.registration_finish_plan([1, 33, 0])["launches"] == \
        capi.robust_registration_batch_plan([33])["launches"] + 1


def test_finish_batch_rows_equal_its_single_calls(capi, ws_host):
    """sage_registration_finish_batch: a row depends on its own problem and scale alone"""
    _, params = ref.load_case("n33")
    probs = _mixed_batch()
    scales = [ref.restated(n)["scale"] for n in BATCH_NAMES]
    scales = scales[:3] + [1.0] + scales[3:] + [1.0, 1.0]
    single = [_np(capi.registration_finish_batch(ws_host, [q], [s], params, device_inliers=True)[0]) for q, s in zip(probs, scales)]
    assert single[7]["valid"] == 0 and single[8]["valid"] == 0 and single[3]["valid"] == 1     # (a scale is given: the row is solved)
    for order in (list(range(len(probs))), list(range(len(probs)))[::-1]):
        out = capi.registration_finish_batch(ws_host, [probs[b] for b in order], [scales[b] for b in order], params, device_inliers=True)
        for row, b in enumerate(order):
            _same_bytes(out[row], single[b], (order[0], b))


# ---- 4. mode isolation
def test_a_new_workspace_is_in_host_mode_and_returns_to_it(capi, ws_host):
    w = capi.Workspace()
    try:
        assert w.registration_finish() == capi.SAGE_REG_FINISH_HOST == 0
        assert capi.workspace_registration_finish_raw(None) == capi.SAGE_REG_FINISH_HOST
        w.set_registration_finish(capi.SAGE_REG_FINISH_DEVICE)
        assert w.registration_finish() == capi.SAGE_REG_FINISH_DEVICE
        q, params = _problem("n64_o30")
        assert capi.robust_registration(w, q["src"], q["dst"], q["noise_bounds"], params)["valid"] == 1
        w.set_registration_finish(capi.SAGE_REG_FINISH_HOST)
        assert w.registration_finish() == capi.SAGE_REG_FINISH_HOST
        for name in ("n64_o30", "n257"):
            q, params = _problem(name)
            back = capi.robust_registration(w, q["src"], q["dst"], q["noise_bounds"], params, device_inliers=True)
            never = capi.robust_registration(ws_host, q["src"], q["dst"], q["noise_bounds"], params, device_inliers=True)
            _same_bytes(back, never, name)
            b2 = capi.robust_registration_batch(w, [q, q], params, device_inliers=True)
            n2 = capi.robust_registration_batch(ws_host, [q, q], params, device_inliers=True)
            assert capi.robust_registration_batch_launches(w) == capi.robust_registration_batch_launches(ws_host)
            for a, b in zip(b2, n2):
                _same_bytes(a, b, name)
    finally:
        w.close()


# ---- 5. the pre-check
def test_precheck_in_device_mode_equals_host_mode(capi, ws, ws_host):
    import torch
    sc = synth.make_loop_candidates(3, 3, K=64)
    assert [c["kind"] for c in sc["cands"]] == ["planted", "self", "unrelated"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    desc_q = cu(sc["desc_q"])
    cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
    params = synth.registration_params(123.0)          # (noise_bound: replaced per candidate)
    run = lambda w: capi.loop_precheck(w, desc_q, sc["depth_divisor"], cands, sc["H"], sc["W"], sc["cam"], 1.0, 2.0, 0.3, params)
    host, dev = run(ws_host), run(ws)
    assert [h["registered"] for h in host] == [1, 1, 0]                 # the unrelated candidate is pruned by the ratio
    for b, (h, d) in enumerate(zip(host, dev)):
        for k in ("n_cycle", "n_matched", "registered"):
            assert h[k] == d[k], (b, k)
        for k in INT_FIELDS:
            assert h["reg"][k] == d["reg"][k], (b, k)
        for k in ("relative_desc_match_inlier_ratio", "desc_match_inlier_ratio", "mean_noise_depth"):
            assert h[k].tobytes() == d[k].tobytes(), (b, k)
        assert np.array_equal(h["inlier_kp"].cpu().numpy(), d["inlier_kp"].cpu().numpy())
        assert np.array_equal(h["raw_matched"].cpu().numpy(), d["raw_matched"].cpu().numpy())
        for k in ("scale", "scale_cost"):                               # (the vote is the same code on the same inputs)
            assert np.float64(h["reg"][k]).tobytes() == np.float64(d["reg"][k]).tobytes(), (b, k)
        if not h["registered"]:
            continue
        assert h["reg"]["n_inliers"] > 0
        # the bounds of the finish for this candidate's gathered points, from the restatement at the voted scale
        g = capi.match_points(ws_host, h["flags"].contiguous(), h["raw_matched"].contiguous(), cands[b]["kp_dpts0"], cands[b]["kp_homo0"],
                              sc["depth_divisor"], cands[b]["dpt_map"], sc["cam"], sc["W"], 2.0, 1)
        nb = (np.float32(2.0) * np.float32(g["mean_depth"])) / ((np.float32(sc["cam"].fx) + np.float32(sc["cam"].fy)) / np.float32(2))
        f = ref.finish(g["pts0"].cpu().numpy(), g["pts1"].cpu().numpy(), g["noise_bounds"].cpu().numpy(), h["reg"]["scale"],
                       dict(params, noise_bound=float(nb)))
        f["scale"] = h["reg"]["scale"]
        n = g["M"]
        assert np.array_equal(g["kept"].cpu().numpy()[f["inliers"]], h["inlier_kp"].cpu().numpy())
        b_R = ref.rotation_bound(f, n); b_t = ref.translation_bound(f, n, b_R, 0.0)
        assert np.abs(h["reg"]["R"] - d["reg"]["R"]).max() <= b_R and np.abs(h["reg"]["t"] - d["reg"]["t"]).max() <= b_t


# ---- 6. arguments
def test_new_calls_check_their_arguments(capi, ws, ws_host):
    q, params = _problem("n33")
    N = 33
    p = capi.registration_params(params)
    prob = (capi.SageRegistrationProblem * 2)(*[capi.SageRegistrationProblem(capi.dptr(q["src"]).value, capi.dptr(q["dst"]).value,
                                                                            capi.dptr(q["noise_bounds"]).value, N, 0.01, None)] * 2)
    res = (capi.SageRegistrationResult * 2)()
    inl = np.full((2, N), -7, np.int32); rot = np.full((2, N), 7, np.uint8)
    scales = np.array([1.0, 1.0])

    def fin(**kw):
        for r in res:
            r.valid = 77
        a = dict(ws=ws_host.h, probs=C.addressof(prob), B=2, scales=scales.ctypes.data, p=C.addressof(p), res=C.addressof(res),
                 inl=inl.ctypes.data, stride=N, rot=rot.ctypes.data)
        a.update(kw)
        return capi.registration_finish_batch_raw(a["ws"], a["probs"], a["B"], a["scales"], a["p"], a["res"], a["inl"], a["stride"], a["rot"])

    untouched = lambda: all(r.valid == 77 for r in res) and bool((inl == -7).all()) and bool((rot == 7).all())
    for bad in (dict(ws=None), dict(probs=None), dict(scales=None), dict(p=None), dict(res=None), dict(B=-1), dict(B=33), dict(stride=N - 1),
                dict(stride=N - 1, inl=None)):
        assert fin(**bad) == -1 and untouched(), bad
    over = capi.registration_params(params, rotation_max_iterations=capi.SAGE_REG_FINISH_MAX_ITERATIONS + 1)
    at = capi.registration_params(params, rotation_max_iterations=capi.SAGE_REG_FINISH_MAX_ITERATIONS)
    assert fin(p=C.addressof(over)) == -2 and untouched()
    fgr = capi.registration_params(params, rotation_algorithm=capi.SAGE_REG_FGR)
    assert fin(p=C.addressof(fgr)) == -2 and untouched()
    assert fin(B=0, ws=None, probs=None, scales=None, p=None, res=None) == 0 and untouched()
    assert fin(p=C.addressof(at)) == 0 and res[0].valid == 1 and res[1].valid == 1            # (the cap itself is accepted)
    assert bytes(res[0]) == bytes(res[1]) and np.array_equal(inl[0], inl[1]) and np.array_equal(rot[0], rot[1])
    # the mode
    assert capi.workspace_set_registration_finish_raw(None, 1) == -1
    for mode in (-1, 2):
        assert capi.workspace_set_registration_finish_raw(ws.h, mode) == -1
    assert ws.registration_finish() == capi.SAGE_REG_FINISH_DEVICE                             # (a refused mode changes nothing)
    # the iteration cap: DEVICE mode refuses before anything is launched, HOST mode accepts
    one = capi.SageRegistrationResult()
    for w, want in ((ws, -2), (ws_host, 0)):
        one.valid = 77
        rc = capi.robust_registration_raw(w.h, capi.dptr(q["src"]), capi.dptr(q["dst"]), capi.dptr(q["noise_bounds"]), N, C.addressof(over),
                                          C.addressof(one), None, None)
        assert rc == want and one.valid == (77 if want else 1)
        res[0].valid = res[1].valid = 77
        launches = capi.robust_registration_batch_launches(w)
        rc = capi.robust_registration_batch_raw(w.h, C.addressof(prob), 2, C.addressof(over), C.addressof(res), None, 0)
        assert rc == want and res[0].valid == (77 if want else 1)
        if want:
            assert capi.robust_registration_batch_launches(w) == launches
    # the plan
    n = np.array([64, 3], np.int32)
    raw = capi.registration_finish_plan_raw
    assert raw(n.ctypes.data, 2, None, None, None, None) == 0 and raw(None, 2, None, None, None, None) == -1
