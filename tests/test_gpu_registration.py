"""sage_robust_registration (the scale vote on the device, the finish on the host) and sage_match_points against the fixtures
the reference's solver wrote (tests/golden/registration_*.npz) and the fp64 restatement of tests/registration_ref.py.

Cases (tests/registration_ref.CASES): N = 2, 3, 33, 64, 257, 512, 1024 -- one pair; the smallest vote; a partial wave; endpoints
straddling a 2048-endpoint tile; many workgroups with nothing aligned; the shipped size (with 50 % outliers); the cap, 2^20 - 1024
endpoints -- and at N = 64 outliers of 0 / 30 / 70 %, all outliers, noise-free input, coincident dst points, coincident src
points (pairs that leave the vote: compared with the restatement without those pairs, the reference has no defined behaviour
there), bounds at the 5e-4 clamp.  tests/test_registration_ref.py shows on the CPU that no fixture has tied endpoint keys and
that every discrete margin is > 1e-6, so the counts, lists and masks are demanded exactly.

Bounds.  scale: relative 4 n_endpoints 2^-53 (sum |w X| / |sum_consensus w X| + the same for the denominator sum w), the bound
of a reordered sum for numerator and denominator of x = sum w X / sum w, computed by the restatement over the endpoints up to
the minimum.  R, t: 8 x the largest change the restatement's finish shows on the CPU when fed scale (1 +- that bound) (the rule
of tests/test_gpu_track_overlap.py).  R depends on the scale only through the GNC's weights: where the GNC leaves at once
(n3, n64_o0, n64_noise_free) that change is the restatement's own rounding, a few 1e-16, and the bound 3e-15 .. 6e-15.
N = 2: the two chain TIMs are antiparallel, the rotation about their direction is open (every SVD picks its own): scale,
counts, lists, and that R maps the src TIM's direction onto the dst TIM's are compared.

Measured on an MI355X: the device's distance from the restatement, and the bounds

  case                 |dscale|/scale -> bound     |dR| -> 8 x change     |dt| -> 8 x change
  n2                   0.00e+00 -> 1.78e-15   (R, t: open at N = 2)
  n3                   0.00e+00 -> 5.33e-15   3.75e-16 -> 3.25e-15   1.06e-16 -> 2.70e-14
  n33                  2.30e-16 -> 1.91e-12   4.58e-16 -> 9.25e-13   5.69e-16 -> 1.82e-11
  n64_o0               6.61e-16 -> 3.58e-12   3.33e-16 -> 3.77e-15   1.17e-15 -> 3.69e-11
  n64_o30              9.12e-16 -> 9.42e-12   4.16e-16 -> 1.56e-12   9.71e-16 -> 7.45e-11
  n64_o70              6.00e-16 -> 2.68e-11   1.55e-15 -> 2.30e-11   2.78e-15 -> 2.01e-10
  n64_all_outliers     3.89e-15 -> 2.85e-10   2.21e-14 -> 1.43e-10   2.98e-14 -> 4.54e-09
  n64_noise_free       4.06e-16 -> 3.58e-12   4.44e-16 -> 6.22e-15   2.08e-16 -> 2.24e-11
  n64_coincident_dst   2.41e-16 -> 8.91e-12   7.77e-16 -> 1.78e-11   2.36e-16 -> 6.26e-11
  n64_coincident_src   5.87e-16 -> 7.36e-12   3.61e-16 -> 1.00e-11   1.35e-15 -> 8.58e-11
  n64_clamp            2.16e-16 -> 7.14e-12   8.88e-16 -> 1.28e-12   3.58e-18 -> 1.39e-12
  n257                 2.62e-16 -> 1.42e-10   3.05e-16 -> 1.04e-10   3.47e-16 -> 9.43e-10
  n512_o50             3.15e-15 -> 7.87e-10   5.55e-16 -> 4.11e-10   2.44e-15 -> 4.78e-09
  n1024                5.79e-15 -> 2.59e-09   1.11e-15 -> 2.91e-10   7.06e-15 -> 2.55e-08
"""
import ctypes as C
import threading

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import registration_ref as ref

pytestmark = pytest.mark.gpu

ALL_CASES = list(ref.CASES)


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


def _device_solve(capi, ws, name, device_inliers=True):
    import torch
    fx, params = ref.load_case(name)
    src, dst, nb = (torch.from_numpy(fx[k]).cuda() for k in ("src", "dst", "noise_bounds"))
    out = capi.robust_registration(ws, src, dst, nb, params, device_inliers=device_inliers)
    if device_inliers:
        out["inliers_dev"] = out["inliers_dev"].cpu().numpy()
    return out


@pytest.mark.parametrize("name", ALL_CASES)
def test_registration_equals_the_fixture(capi, ws, name):
    from tests.conftest import summary_line
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    n = fx["src"].shape[0]
    d = _device_solve(capi, ws, name)
    exp_inliers = fx["ref_inliers"] if bool(fx["reference"]) else r["inliers"]
    exp_scale_pairs = int(fx["ref_n_scale_inlier_pairs"]) if bool(fx["reference"]) else r["n_scale_inlier_pairs"]
    exp_rot = int(fx["ref_rotation_mask"].sum()) if bool(fx["reference"]) else r["n_rotation_inliers"]
    assert d["valid"] == 1
    assert d["n_pairs"] == n * (n - 1) // 2 and d["n_degenerate_pairs"] == r["n_degenerate_pairs"]
    assert d["n_scale_inlier_pairs"] == exp_scale_pairs
    assert d["n_inliers"] == exp_inliers.size and np.array_equal(d["inliers"], exp_inliers) and np.array_equal(d["inliers_dev"], exp_inliers)
    assert d["n_rotation_inliers"] == exp_rot
    assert d["rotation_iterations"] == r["rotation_iterations"]   # (the reference does not expose it: the restatement's, whose
    #                                                               cost at termination equals the fixture's: test_registration_ref.py)
    if name == "n64_coincident_src":
        assert d["n_degenerate_pairs"] > 0
    b_s = r["bound"]
    d_s = abs(d["scale"] - r["scale"]) / abs(r["scale"])
    assert d_s <= b_s, (d_s, b_s)
    assert abs(d["scale_cost"] - r["scale_cost"]) <= 1e-9 * abs(r["scale_cost"]) + 1e-12   # (well inside the gap to the second cost)
    if n == 2:
        u_s = fx["src"][1].astype(np.float64) - fx["src"][0]; u_d = fx["dst"][1].astype(np.float64) - fx["dst"][0]
        assert np.allclose(d["R"] @ d["R"].T, np.eye(3), atol=1e-12) and np.linalg.det(d["R"]) > 0
        assert np.allclose(d["R"] @ (u_s / np.linalg.norm(u_s)), u_d / np.linalg.norm(u_d), atol=1e-12)
        summary_line(f"registration {name:20s} {d_s:.2e} -> {b_s:.2e}   (R, t: open at N = 2)")
        return
    ch_R = ch_t = 0.0
    for s in (r["scale"] * (1 + b_s), r["scale"] * (1 - b_s)):
        f = ref.finish(fx["src"], fx["dst"], fx["noise_bounds"], s, params)
        assert np.array_equal(f["inliers"], r["inliers"])
        ch_R = max(ch_R, np.abs(f["R"] - r["R"]).max()); ch_t = max(ch_t, np.abs(f["t"] - r["t"]).max())
    d_R = np.abs(d["R"] - r["R"]).max(); d_t = np.abs(d["t"] - r["t"]).max()
    summary_line(f"registration {name:20s} {d_s:.2e} -> {b_s:.2e}   {d_R:.2e} -> {8 * ch_R:.2e}   {d_t:.2e} -> {8 * ch_t:.2e}")
    assert d_R <= 8 * ch_R and d_t <= 8 * ch_t


def test_repeated_and_interleaved_calls_return_identical_bytes(capi, ws):
    """the workspace's buffers are reused across sizes: a small problem after the cap's, then the cap's again"""
    first = {n: _device_solve(capi, ws, n) for n in ("n1024", "n3", "n257")}
    for n in ("n3", "n1024", "n257"):
        again = _device_solve(capi, ws, n)
        for k in first[n]:
            assert np.array_equal(np.asarray(first[n][k]), np.asarray(again[k])), (n, k)


def test_fewer_than_two_points_and_bad_arguments(capi, ws):
    import torch
    fx, params = ref.load_case("n33")
    src, dst, nb = (torch.from_numpy(fx[k]).cuda() for k in ("src", "dst", "noise_bounds"))
    p = capi.registration_params(params)
    res = capi.SageRegistrationResult()
    inl = np.full(33, -7, np.int32)
    raw = lambda **kw: capi.robust_registration_raw(kw.get("ws", ws.h), kw.get("src", capi.dptr(src)), kw.get("dst", capi.dptr(dst)),
                                                    kw.get("nb", capi.dptr(nb)), kw.get("N", 33), kw.get("p", C.addressof(p)),
                                                    kw.get("res", C.addressof(res)), inl.ctypes.data, None)
    for N in (0, 1):
        res.valid = 5; res.n_inliers = 5
        assert raw(N=N) == 0 and res.valid == 0 and res.n_inliers == 0 and np.all(inl == -7)
    for bad in (dict(ws=None), dict(src=None), dict(dst=None), dict(nb=None), dict(p=None), dict(res=None), dict(N=-1), dict(N=1025)):
        assert raw(**bad) == -1, bad
    for field, value in (("rotation_tim_graph", capi.SAGE_REG_COMPLETE), ("inlier_selection_mode", capi.SAGE_REG_SELECT_PMC_EXACT),
                         ("inlier_selection_mode", capi.SAGE_REG_SELECT_PMC_HEU), ("inlier_selection_mode", capi.SAGE_REG_SELECT_KCORE_HEU),
                         ("rotation_algorithm", capi.SAGE_REG_FGR)):
        q = capi.registration_params(params, **{field: value})
        assert raw(p=C.addressof(q)) == -2, field
    q = capi.registration_params(params, cbar2=0.0)
    assert raw(p=C.addressof(q)) == -1
    assert raw() == 0 and res.valid == 1 and res.n_inliers == ref.restated("n33")["n_inliers"]   # the workspace still works
    # every pair degenerate: nothing is left in the vote
    same = torch.zeros(5, 3, device="cuda")
    out = capi.robust_registration(ws, same, same.clone(), torch.full((5,), 0.01, device="cuda"), params)
    assert out["valid"] == 0 and out["n_pairs"] == 10 and out["n_degenerate_pairs"] == 10 and out["n_inliers"] == 0


def test_two_workspaces_on_two_threads_equal_one(capi, ws):
    """the contract of tests/test_gpu_threads.py: own workspace per host thread, bit-identical results"""
    import torch
    names = ("n64_o30", "n257", "n512_o50")
    single = {n: _device_solve(capi, ws, n) for n in names}
    results, errors = [dict(), dict()], []

    def worker(slot, stream):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(stream):   # (None: the default stream; torch's own fills and copies go where the workspace's do)
                w = capi.Workspace(stream)
                for _ in range(3):
                    for n in names:
                        results[slot][n] = _device_solve(capi, w, n)
                w.close()
        except Exception as e:   # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(0, None)), threading.Thread(target=worker, args=(1, torch.cuda.Stream()))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for slot in (0, 1):
        for n in names:
            for k in single[n]:
                assert np.array_equal(np.asarray(single[n][k]), np.asarray(results[slot][n][k])), (slot, n, k)


# ---- the gather
class _Cam:
    fx, fy, cx, cy, w, h = 61.5, 59.25, 31.5, 23.75, 64.0, 48.0


def _gather_problem(K, pattern, seed=0):
    rng = np.random.default_rng([seed, K])
    H, W = 48, 64
    flags = {"all": np.ones(K, np.int32), "none": np.zeros(K, np.int32), "alternating": (np.arange(K) % 2).astype(np.int32)}[pattern]
    return dict(flags=flags, loc1=rng.integers(0, H * W, K).astype(np.int64), dpts0=rng.uniform(0.3, 3.0, K).astype(np.float32),
                homo0=np.concatenate([rng.uniform(-0.5, 0.5, (K, 2)), np.ones((K, 1))], 1).astype(np.float32),
                dmap1=rng.uniform(0.01, 3.0, H * W).astype(np.float32), W=W)


def _gather_torch_cpu(g, cam, divisor, mult, noise_from):
    """the reference's tensor expressions (camera_tracker.cpp:654-714) on the CPU"""
    import torch
    t = {k: torch.from_numpy(v) for k, v in g.items() if k != "W"}
    idx = torch.nonzero(t["flags"]).reshape(-1)
    h0 = t["homo0"][idx]; d0 = t["dpts0"][idx]; loc = t["loc1"][idx]
    x = torch.fmod(loc, float(g["W"])); y = torch.floor(loc / float(g["W"]))
    hx = (x - cam.cx) / cam.fx; hy = (y - cam.cy) / cam.fy
    homo1 = torch.stack([hx, hy, torch.ones_like(hx)], 1)
    d1 = t["dmap1"][loc]
    pts0 = d0.reshape(-1, 1) / divisor * h0
    pts1 = d1.reshape(-1, 1) * homo1
    focal = float(np.float32((np.float32(cam.fx) + np.float32(cam.fy)) / 2.0))
    d = d1 if noise_from else d0
    nb = torch.clamp_min(mult * d / focal, 5.0e-4)
    assert x.dtype == torch.float32 and nb.dtype == torch.float32
    return dict(kept=idx.to(torch.int32), pts0=pts0, pts1=pts1, homo1=homo1, dpts1=d1, noise_bounds=nb,
                mean64=float(d.double().mean()) if idx.numel() else 0.0)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 512])
def test_match_points_equals_the_tensor_expressions(capi, ws, K, pattern):
    import torch
    g = _gather_problem(K, pattern)
    for noise_from, divisor in ((1, 1.7), (0, 1.0)):
        e = _gather_torch_cpu(g, _Cam, divisor, 2.0, noise_from)
        dev = {k: torch.from_numpy(v).cuda() for k, v in g.items() if k != "W"}
        o = capi.match_points(ws, dev["flags"], dev["loc1"], dev["dpts0"], dev["homo0"], divisor, dev["dmap1"], _Cam, g["W"], 2.0, noise_from)
        assert o["M"] == int(g["flags"].sum())
        for k in ("kept", "pts0", "pts1", "homo1", "dpts1", "noise_bounds"):
            a, b = o[k].cpu().numpy(), e[k].numpy()
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, noise_from)
        if o["M"]:
            assert abs(float(o["mean_depth"]) - e["mean64"]) <= 2.0 ** -24 * abs(e["mean64"])


def test_match_points_checks_its_arguments(capi, ws):
    import torch
    g = _gather_problem(8, "all")
    dev = {k: torch.from_numpy(v).cuda() for k, v in g.items() if k != "W"}
    cam = capi.SageCamera(_Cam.fx, _Cam.fy, _Cam.cx, _Cam.cy, _Cam.w, _Cam.h)
    out3, pts1, homo1 = (torch.zeros(8, 3, device="cuda") for _ in range(3))
    out1, dpts1 = (torch.zeros(8, device="cuda") for _ in range(2))
    kept = torch.zeros(8, dtype=torch.int32, device="cuda")
    M = C.c_int(-1)

    def raw(**kw):
        a = dict(ws=ws.h, flags=capi.dptr(dev["flags"]), loc=capi.dptr(dev["loc1"]), d0=capi.dptr(dev["dpts0"]), h0=capi.dptr(dev["homo0"]),
                 dm=capi.dptr(dev["dmap1"]), cam=C.addressof(cam), K=8, W=64, nf=1, pts0=capi.dptr(out3), M=C.addressof(M))
        a.update(kw)
        return capi.match_points_raw(a["ws"], a["flags"], a["loc"], a["d0"], a["h0"], 1.0, a["dm"], a["cam"], a["K"], a["W"], 2.0, a["nf"],
                                     a["pts0"], capi.dptr(pts1), capi.dptr(out1), capi.dptr(homo1), capi.dptr(dpts1),
                                     capi.dptr(kept), a["M"], None)
    assert raw() == 0 and M.value == 8
    for bad in (dict(ws=None), dict(flags=None), dict(loc=None), dict(d0=None), dict(h0=None), dict(dm=None), dict(cam=None), dict(K=0),
                dict(W=0), dict(nf=2), dict(pts0=None), dict(M=None)):
        assert raw(**bad) == -1, bad
    # a location outside the image reads a NaN depth instead of memory
    loc = dev["loc1"].clone(); loc[3] = 48 * 64; loc[5] = -1
    o = capi.match_points(ws, dev["flags"], loc, dev["dpts0"], dev["homo0"], 1.0, dev["dmap1"], _Cam, 64, 2.0, 1)
    d1 = o["dpts1"].cpu().numpy()
    assert np.isnan(d1[3]) and np.isnan(d1[5]) and np.isfinite(np.delete(d1, [3, 5])).all()


# ---- the chain: descriptors -> cycle match -> gather -> registration -> the tracker's keypoint operator
def _chain_scene(seed=3):
    """48x64, 16 descriptor channels.  Keypoints on a 4-pixel grid of frame 0 with a smooth depth; frame 1 sees them under a
    planted (s, R, t): each keypoint's descriptor is planted at the pixel its point projects to (rounded: up to half a pixel,
    a quarter of the bound 2 d / f), with that point's depth in frame 1's depth map; 8 keypoints are planted at a wrong pixel"""
    rng = np.random.default_rng(seed)
    H, W, Cd = 48, 64, 16
    fx = fy = 60.0; cx, cy = 31.5, 23.5
    ys, xs = np.meshgrid(np.arange(8, 41, 4), np.arange(8, 57, 4), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    K = xs.size
    d0 = (1.5 + 0.3 * np.sin(xs / 9.0) + 0.2 * np.cos(ys / 7.0)).astype(np.float32)
    homo0 = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(K)], 1).astype(np.float32)
    s = 1.2; R = synth.so3_exp(np.array([0.02, -0.03, 0.025])); t = np.array([0.03, -0.02, 0.04])
    p1 = s * (d0[:, None].astype(np.float64) * homo0) @ R.T + t
    u1 = np.rint(p1[:, 0] / p1[:, 2] * fx + cx).astype(np.int64); v1 = np.rint(p1[:, 1] / p1[:, 2] * fy + cy).astype(np.int64)
    wrong = rng.permutation(K)[:8]
    free = np.array([[x, y] for y in range(2, H - 2) for x in range(2, W - 2) if (x % 4 == 1 and y % 4 == 1)])
    pick = free[rng.permutation(len(free))[:8]]
    u1[wrong], v1[wrong] = pick[:, 0], pick[:, 1]
    assert u1.min() >= 0 and u1.max() < W and v1.min() >= 0 and v1.max() < H
    loc1 = v1 * W + u1
    assert np.unique(loc1).size == K
    desc0 = rng.normal(0, 1, (Cd, H, W)).astype(np.float32); desc1 = rng.normal(0, 1, (Cd, H, W)).astype(np.float32)
    desc1[:, v1, u1] = desc0[:, ys, xs]
    dmap1 = np.full(H * W, 2.0, np.float32)
    dmap1[loc1] = p1[:, 2].astype(np.float32)
    dmap1[loc1[wrong]] = rng.uniform(1.0, 3.0, 8).astype(np.float32)
    cam = type("Cam", (), dict(fx=fx, fy=fy, cx=cx, cy=cy, w=float(W), h=float(H)))
    return dict(H=H, W=W, K=K, kp_loc0=(ys * W + xs).astype(np.int64), loc1=loc1, d0=d0, homo0=homo0, desc0=desc0, desc1=desc1, dmap1=dmap1,
                cam=cam, s=s, R=R, t=t, wrong=np.sort(wrong))


def test_chain_from_descriptors_to_the_keypoint_operator(capi, ws):
    import torch
    sc = _chain_scene()
    cu = lambda a: torch.from_numpy(a).cuda()
    raw1, cyc0, flags, n_cyc = capi.cycle_match(ws, cu(sc["desc0"]), cu(sc["desc1"]), cu(sc["kp_loc0"]), sc["H"], sc["W"], 1.0)
    assert n_cyc == sc["K"] and np.array_equal(raw1.cpu().numpy(), sc["loc1"])
    g = capi.match_points(ws, flags.contiguous(), raw1.contiguous(), cu(sc["d0"]), cu(sc["homo0"]), 1.0, cu(sc["dmap1"]), sc["cam"], sc["W"], 2.0, 1)
    assert g["M"] == sc["K"]
    noise_bound = 2.0 * float(g["mean_depth"]) / 60.0
    out = capi.robust_registration(ws, g["pts0"].contiguous(), g["pts1"].contiguous(), g["noise_bounds"].contiguous(),
                                   synth.registration_params(noise_bound), device_inliers=True)
    assert out["valid"] == 1
    inl = out["inliers"]
    assert not np.intersect1d(inl, sc["wrong"]).size and inl.size >= 0.8 * (sc["K"] - 8)
    # within the noise bound of the plant: for every inlier the recovered transform and the planted one put its point within
    # 1.25 x its bound of each other per axis (1 from the translation vote, 0.25 from the pixel rounding of the plant)
    p0 = g["pts0"].cpu().numpy().astype(np.float64)[inl]; nb = g["noise_bounds"].cpu().numpy().astype(np.float64)[inl]
    rec = out["scale"] * p0 @ out["R"].T + out["t"]; planted = sc["s"] * p0 @ sc["R"].T + sc["t"]
    assert np.all(np.abs(rec - planted) <= 1.25 * nb[:, None] + 1e-6)
    # ... and with it the scale: two inliers a, b give | |s R (a - b)| - |s' R' (a - b)| | = |s - s'| |a - b| <= 2 sqrt(3) 1.25 nb
    spread = np.linalg.norm(p0 - p0.mean(0), axis=1).max()
    assert abs(out["scale"] - sc["s"]) <= 2 * np.sqrt(3.0) * 1.25 * nb.max() / spread
    # the operator on the compacted arrays
    idx = out["inliers_dev"].long()
    args = [g[k][idx].contiguous() for k in ("dpts1",)]
    d0c = cu(sc["d0"])[g["kept"].long()][idx].contiguous(); h0c = cu(sc["homo0"])[g["kept"].long()][idx].contiguous()
    h1c = g["homo1"][idx].contiguous()
    Rf = torch.from_numpy(out["R"].astype(np.float32)).cuda().contiguous(); tf = torch.from_numpy(out["t"].astype(np.float32)).cuda().contiguous()
    d0s = (d0c * float(out["scale"])).contiguous()   # (the tracker hands the operator depths scaled for the evaluation)
    at_solution = capi.tracker_match_geom(ws, True, True, Rf, tf, d0s, args[0], h0c, h1c, float(out["scale"]), 0.1, 1.0)
    eye = torch.eye(3, device="cuda").contiguous(); zero = torch.zeros(3, device="cuda")
    at_identity = capi.tracker_match_geom(ws, True, True, eye, zero, d0c, args[0], h0c, h1c, 1.0, 0.1, 1.0)
    assert np.isfinite(at_solution["error"]) and torch.isfinite(at_solution["AtA"]).all() and at_solution["AtA"].shape == (7, 7)
    assert at_solution["error"] < at_identity["error"]
