"""sage_loop_precheck on the batched gather and the batched registration: B candidates, four waits, and per candidate the
bytes of the three single calls.

Scenes (synth.make_loop_candidates): 32 x 40 with K = 24 keypoints and 48 x 64 with K = 117, B = 1, 5 and 20, the kinds in turn
planted / self / unrelated / planted, and from B = 5 on one candidate more, "one match": the unrelated candidate's maps with a
keypoint set made of ONE keypoint whose cycle closes and, repeated, keypoints whose cycle does not (the cycle match looks at
every keypoint by itself), so that the gather keeps M = 1 and the solve is skipped.  Two thresholds: 0.3 prunes the unrelated
candidates before the gather, 0 lets everything with a cycle match through to the gather.

The comparison is that of tests/test_gpu_loop_precheck.py::same_as_single, restated: identical values, identical bytes."""
import numpy as np
import pytest

from sage_slam_amd import synth

pytestmark = pytest.mark.gpu

CYC_THRESH, MULT = 1.0, 2.0
SCENES = {"32x40": dict(H=32, W=40, K=24), "48x64": dict(H=48, W=64, K=117)}


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


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _one_match_candidate(capi, ws, desc_q, cand, H, W):
    """-> the candidate with its keypoints replaced as the docstring says, or None when no cycle closes / all do"""
    import torch
    raw, cyc, flags, n = capi.cycle_match(ws, desc_q, cand["desc"], cand["kp_loc"], H, W, CYC_THRESH)
    hit = flags.nonzero().reshape(-1); miss = (flags == 0).nonzero().reshape(-1)
    if hit.numel() == 0 or miss.numel() == 0:
        return None
    K = int(flags.numel())
    sel = torch.cat([hit[:1], miss.repeat(K)[:K - 1]])
    assert sel.numel() == K
    return dict(desc=cand["desc"], dpt_map=cand["dpt_map"], kp_loc=cand["kp_loc"][sel].contiguous(), kp_dpts0=cand["kp_dpts0"][sel].contiguous(),
                kp_homo0=cand["kp_homo0"][sel].contiguous())


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request, capi, ws):
    """20 candidates of one scene on the device (a batch of B takes the first B), and the single calls' answers, once"""
    s = SCENES[request.param]
    sc = synth.make_loop_candidates(5, 20, H=s["H"], W=s["W"], K=s["K"])
    desc_q = _cu(sc["desc_q"])
    cands = [{k: _cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
    one = _one_match_candidate(capi, ws, desc_q, cands[2], sc["H"], sc["W"])
    assert one is not None, "the unrelated candidate closes no cycle or all of them: pick another seed"
    cands[4] = one                                                  # (B = 5 and 20 hold it)
    single = []
    cam = sc["cam"]
    for c in cands:
        raw, cyc, flags, n_cyc = capi.cycle_match(ws, desc_q, c["desc"], c["kp_loc"], sc["H"], sc["W"], CYC_THRESH)
        r = dict(n_cycle=n_cyc, raw=raw.cpu().numpy(), flags=flags.cpu().numpy(), n_matched=0, mean_depth=np.float32(0), reg=None)
        if n_cyc > 0:
            g = capi.match_points(ws, flags.contiguous(), raw.contiguous(), c["kp_dpts0"], c["kp_homo0"], sc["depth_divisor"], c["dpt_map"],
                                  cam, sc["W"], MULT, 1)
            nb = (np.float32(MULT) * np.float32(g["mean_depth"])) / ((np.float32(cam.fx) + np.float32(cam.fy)) / np.float32(2))
            assert nb.dtype == np.float32
            r.update(n_matched=g["M"], mean_depth=g["mean_depth"])
            if g["M"] >= 2 and nb > 0 and np.isfinite(nb):
                reg = capi.robust_registration(ws, g["pts0"].contiguous(), g["pts1"].contiguous(), g["noise_bounds"].contiguous(),
                                               synth.registration_params(float(nb)))
                r.update(reg=reg, inlier_kp=g["kept"].cpu().numpy()[reg["inliers"]])
        single.append(r)
    assert single[4]["n_cycle"] == 1 and single[4]["n_matched"] == 1 and single[4]["reg"] is None
    return dict(sc=sc, desc_q=desc_q, cands=cands, single=single, K=s["K"])


def precheck(capi, ws, scene, B, min_ratio):
    sc = scene["sc"]
    return capi.loop_precheck(ws, scene["desc_q"], sc["depth_divisor"], scene["cands"][:B], sc["H"], sc["W"], sc["cam"], CYC_THRESH, MULT,
                              min_ratio, synth.registration_params(123.0))       # (noise_bound: replaced per candidate)


def same_as_single(got, want, K, min_ratio):
    """every field and every output row of one candidate against the composition of the single calls"""
    assert got["n_cycle"] == want["n_cycle"]
    assert np.array_equal(got["raw_matched"].cpu().numpy(), want["raw"]) and np.array_equal(got["flags"].cpu().numpy(), want["flags"])
    pruned = want["n_cycle"] <= 0 or np.float32(want["n_cycle"]) / np.float32(K) < np.float32(min_ratio)
    g = got["reg"]
    if pruned or want["reg"] is None:
        assert got["registered"] == 0 and got["relative_desc_match_inlier_ratio"] == 0 and got["desc_match_inlier_ratio"] == 0
        assert g["valid"] == 0 and g["n_inliers"] == 0 and g["n_pairs"] == 0 and g["scale"] == 0 and got["inlier_kp"].numel() == 0
        assert got["n_matched"] == (0 if pruned else want["n_matched"])
        assert got["mean_noise_depth"].tobytes() == np.float32(0 if pruned else want["mean_depth"]).tobytes()
        return "pruned" if pruned else "not solved"
    assert got["registered"] == 1 and got["n_matched"] == want["n_matched"]
    assert got["mean_noise_depth"].tobytes() == np.float32(want["mean_depth"]).tobytes()
    w = want["reg"]
    for k in ("valid", "n_inliers", "n_pairs", "n_degenerate_pairs", "n_scale_inlier_pairs", "rotation_iterations", "n_rotation_inliers"):
        assert g[k] == w[k], k
    for k in ("scale", "scale_cost"):
        assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), k
    assert g["R"].tobytes() == w["R"].tobytes() and g["t"].tobytes() == w["t"].tobytes()
    assert got["relative_desc_match_inlier_ratio"] == np.float32(w["n_inliers"]) / np.float32(want["n_matched"])
    assert got["desc_match_inlier_ratio"] == np.float32(w["n_inliers"]) / np.float32(K)
    assert np.array_equal(got["inlier_kp"].cpu().numpy(), want["inlier_kp"])
    return "registered"


@pytest.mark.parametrize("min_ratio", [0.3, 0.0])
@pytest.mark.parametrize("B", [1, 5, 20])
def test_every_candidate_equals_the_three_single_calls(capi, ws, scene, B, min_ratio):
    res = precheck(capi, ws, scene, B, min_ratio)
    assert len(res) == B
    ends = [same_as_single(res[b], scene["single"][b], scene["K"], min_ratio) for b in range(B)]
    assert ends[0] == "registered"                                               # the planted candidate
    if B >= 5:
        assert ends[1] == "registered" and ends[3] == "registered"
        assert ends[4] == ("pruned" if min_ratio > 0 else "not solved")          # one match: M = 1
        assert ends[2] == "pruned" if min_ratio > 0 else ends[2] in ("registered", "not solved", "pruned")
    if B == 20 and min_ratio > 0:
        assert ends.count("pruned") >= 5 and ends.count("registered") >= 10      # the kinds are mixed as the docstring says


def test_a_small_batch_after_a_large_one_shows_no_stale_rows(capi, ws, scene):
    big = precheck(capi, ws, scene, 20, 0.0)
    small = precheck(capi, ws, scene, 3, 0.0)
    assert len(big) == 20 and len(small) == 3
    for b in range(3):
        same_as_single(small[b], scene["single"][b], scene["K"], 0.0)
    again = precheck(capi, ws, scene, 20, 0.0)
    for b in range(20):
        same_as_single(again[b], scene["single"][b], scene["K"], 0.0)
