"""sage_robust_registration_batch and sage_match_points_batch against the single calls.

The contract of include/sage_ba.h: row b of a batch holds, byte for byte, what sage_robust_registration writes for problem b
alone -- whatever else is in the batch, in whatever order, for every SAGE_REG_SORT_TILE.  So every comparison here is for
equality of bytes: every field of SageRegistrationResult, every inlier row (host and device).

Sizes: the fixtures of tests/golden (N = 2 .. 1024: one pair up to the cap, with P from 4 096 to 2^20 in one batch: every sort
stage runs over another prefix of the segments); N = 91 / 92, which straddle P = 8 192 / 16 384; 32 x N = 46, 1 035 pairs each:
two scan tiles, the second holding 22 endpoints, and the batch's cap."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import registration_ref as ref
from tests import test_gpu_registration as single_tests

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["n2", "n3", "n33", "n64_o30", "n64_coincident_src", "n64_all_outliers", "n257", "n1024"]
SHUFFLE = [5, 2, 7, 0, 3, 6, 1, 4]
MIXED = [(257, 0), (0, 0), (46, 1), (91, 2), (1, 0), (92, 3), (33, 4)]       # (N, seed): the mixed batch of the launch and tile tests


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


def _cuda(arrays, noise_bound):
    import torch
    p = {k: torch.from_numpy(np.ascontiguousarray(arrays[k])).cuda() for k in ("src", "dst", "noise_bounds")}
    p["noise_bound"] = float(noise_bound)
    return p


def fixture_problem(name):
    fx, params = ref.load_case(name)
    return _cuda(fx, params["noise_bound"])


def synth_problem(N, seed, variant="plain"):
    if N < 2:                                                     # (does not vote: the arrays are never read)
        z = dict(src=np.zeros((N, 3), np.float32), dst=np.zeros((N, 3), np.float32), noise_bounds=np.full(N, 0.01, np.float32))
        return _cuda(z, 0.01)
    q = synth.make_registration_problem(N, seed, variant=variant)
    return _cuda(q, q["params"]["noise_bound"])


def single(capi, ws, prob):
    out = capi.robust_registration(ws, prob["src"], prob["dst"], prob["noise_bounds"], synth.registration_params(prob["noise_bound"]),
                                   device_inliers=True)
    out["inliers_dev"] = out["inliers_dev"].cpu().numpy()
    return out


def batch(capi, ws, probs, noise_bound=123.0):
    """(the params' own noise_bound is never read: every problem brings its own)"""
    out = capi.robust_registration_batch(ws, probs, synth.registration_params(noise_bound), device_inliers=True)
    for o in out:
        o["inliers_dev"] = o["inliers_dev"].cpu().numpy()
    return out


def same_bytes(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def fixture_probs():
    return [fixture_problem(n) for n in FIXTURES]


@pytest.fixture(scope="module")
def fixture_single(capi, ws, fixture_probs):
    return [single(capi, ws, p) for p in fixture_probs]


@pytest.fixture(scope="module")
def fixture_batch(capi, ws, fixture_probs):
    return batch(capi, ws, fixture_probs)


def test_a_batch_of_the_fixtures_equals_the_single_calls(capi, ws, fixture_single, fixture_batch):
    for name, got, want in zip(FIXTURES, fixture_batch, fixture_single):
        same_bytes(got, want, name)
        assert np.array_equal(got["inliers_dev"], got["inliers"])
        assert got["valid"] == 1


@pytest.mark.parametrize("name", FIXTURES)
def test_a_row_of_the_batch_meets_the_fixtures_expectations(capi, ws, fixture_batch, name, monkeypatch):
    """the checks of tests/test_gpu_registration.py::test_registration_equals_the_fixture, fed the batch's row"""
    row = fixture_batch[FIXTURES.index(name)]
    monkeypatch.setattr(single_tests, "_device_solve", lambda capi_, ws_, name_, device_inliers=True: dict(row))
    single_tests.test_registration_equals_the_fixture(capi, ws, name)


def test_the_order_of_the_batch_does_not_show(capi, ws, fixture_probs, fixture_single):
    for order in (list(range(len(FIXTURES)))[::-1], SHUFFLE):
        got = batch(capi, ws, [fixture_probs[i] for i in order])
        for row, i in enumerate(order):
            same_bytes(got[row], fixture_single[i], (order, FIXTURES[i]))


def test_a_batch_of_one(capi, ws):
    for N, seed in ((64, 0), (257, 1), (2, 2)):
        p = synth_problem(N, seed)
        same_bytes(batch(capi, ws, [p])[0], single(capi, ws, p), N)


def test_two_problems_that_straddle_a_power_of_two(capi, ws):
    probs = [synth_problem(91, 0), synth_problem(92, 0)]
    assert capi.robust_registration_batch_plan([91, 92])["order"] == [1, 0]
    want = [single(capi, ws, p) for p in probs]
    for order in ((0, 1), (1, 0)):
        got = batch(capi, ws, [probs[i] for i in order])
        for row, i in enumerate(order):
            same_bytes(got[row], want[i], (order, i))
            assert got[row]["valid"] == 1 and got[row]["n_pairs"] == (4095, 4186)[i]


def test_the_cap_of_32_problems_against_32_fresh_solves(capi, ws):
    probs = [synth_problem(46, seed) for seed in range(32)]
    got = batch(capi, ws, probs)
    assert len({g["scale"] for g in got}) == 32                    # (32 different problems)
    for seed, (g, p) in enumerate(zip(got, probs)):
        same_bytes(g, single(capi, ws, p), seed)
        assert g["valid"] == 1 and g["n_pairs"] == 1035


def test_a_problem_does_not_see_its_neighbours(capi, ws):
    x = synth_problem(64, 11)
    want = single(capi, ws, x)
    a = batch(capi, ws, [synth_problem(257, 1), x, synth_problem(33, 2)])
    b = batch(capi, ws, [synth_problem(46, 3), synth_problem(64, 4, "all_outliers"), synth_problem(512, 5), x])
    same_bytes(a[1], want, "first neighbours")
    same_bytes(b[3], want, "second neighbours")
    twice = batch(capi, ws, [x, synth_problem(92, 6), x])
    same_bytes(twice[0], want, "twice, first")
    same_bytes(twice[2], want, "twice, second")


def test_problems_that_do_not_vote(capi, ws):
    import torch
    healthy = synth_problem(64, 7)
    want = single(capi, ws, healthy)
    got = batch(capi, ws, [synth_problem(0, 0), healthy, synth_problem(1, 0)])
    same_bytes(got[1], want, "next to N = 0 and N = 1")
    for b in (0, 2):
        assert got[b]["valid"] == 0 and got[b]["n_inliers"] == 0 and got[b]["n_pairs"] == 0 and got[b]["inliers"].size == 0
        assert got[b]["scale"] == 0 and not got[b]["R"].any() and not got[b]["t"].any()
    # an empty vote: every src point is the same point, every pair is degenerate
    same = torch.zeros(5, 3, device="cuda")
    empty = dict(src=same, dst=same.clone(), noise_bounds=torch.full((5,), 0.01, device="cuda"), noise_bound=0.01)
    want_empty = single(capi, ws, empty)
    assert want_empty["valid"] == 0 and want_empty["n_pairs"] == 10 and want_empty["n_degenerate_pairs"] == 10
    for probs, at in (([empty, healthy], (0, 1)), ([healthy, empty], (1, 0)), ([synth_problem(257, 1), empty, healthy], (1, 2))):
        got = batch(capi, ws, probs)
        same_bytes(got[at[0]], want_empty, "the empty vote")
        same_bytes(got[at[1]], want, "next to an empty vote")
    # nothing votes: no launch
    batch(capi, ws, [healthy])
    assert capi.robust_registration_batch_launches(ws) > 0
    got = batch(capi, ws, [synth_problem(1, 0), synth_problem(0, 0), synth_problem(1, 1)])
    assert capi.robust_registration_batch_launches(ws) == 0
    assert all(g["valid"] == 0 and g["n_inliers"] == 0 for g in got)


def _without_device_inliers(capi, ws, probs):
    return capi.robust_registration_batch(ws, probs, synth.registration_params(1.0))


def test_the_call_spends_the_launches_the_plan_states(capi, ws):
    mixed = [synth_problem(N, seed) for N, seed in MIXED[:5]]
    for probs in ([synth_problem(64, 0)], mixed, [synth_problem(46, seed) for seed in range(32)]):
        Ns = [int(p["src"].shape[0]) for p in probs]
        _without_device_inliers(capi, ws, probs)
        spent = capi.robust_registration_batch_launches(ws)
        assert spent == capi.robust_registration_batch_plan(Ns)["launches"] > 0, Ns
        # ... which is what its largest problem alone takes, and one more with company: a batch in which ONE problem votes
        # takes the single call's path, whose publish kernel posts the ticket itself
        voters = len([n for n in Ns if n >= 2])
        assert spent == capi.robust_registration_batch_plan([max(Ns)])["launches"] + (voters > 1)
        if voters > 1:
            assert spent == capi.robust_registration_batch_plan([max(Ns), 2])["launches"]        # (in any company)
    # with inliers_dev rows: one copy launch and its ticket more
    batch(capi, ws, mixed)
    assert capi.robust_registration_batch_launches(ws) == capi.robust_registration_batch_plan([n for n, _ in MIXED[:5]])["launches"] + 2


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sage_slam_amd import capi
from tests.test_gpu_registration_batch import MIXED, synth_problem, batch
ws = capi.Workspace()
rows = batch(capi, ws, [synth_problem(N, seed) for N, seed in MIXED])
print(json.dumps(dict(launches=capi.robust_registration_batch_launches(ws),
                      rows=[{k: np.asarray(v).tobytes().hex() for k, v in sorted(r.items())} for r in rows])))
ws.close()
"""


@pytest.mark.parametrize("tile", [2048, 4096])
def test_another_sort_tile_gives_the_same_bytes(capi, ws, tile):
    """SAGE_REG_SORT_TILE is read per call, but a fresh child process per value keeps this process's environment as it is"""
    want = batch(capi, ws, [synth_problem(N, seed) for N, seed in MIXED])
    env = dict(os.environ, SAGE_REG_SORT_TILE=str(tile))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got["rows"]) == len(want)
    for g, w in zip(got["rows"], want):
        assert g == {k: np.asarray(v).tobytes().hex() for k, v in sorted(w.items())}
    # (fewer launches with a larger tile: P = 65 536 at N = 257)
    assert got["launches"] < capi.robust_registration_batch_launches(ws)


# ---- the gather
@pytest.mark.parametrize("K", [1, 63, 65, 512])
def test_match_points_batch_equals_the_single_calls(capi, ws, K):
    import torch
    cam = single_tests._Cam
    patterns = ["all", "none", "alternating", "none", "alternating", "all"]
    gs = [single_tests._gather_problem(K, pat, seed) for seed, pat in enumerate(patterns)]
    names = dict(flags="flags", loc1="raw_matched_loc1", dpts0="dpts0", homo0="homo0", dmap1="dpt_map_1")
    probs = [{names[k]: torch.from_numpy(v).cuda() for k, v in g.items() if k != "W"} for g in gs]
    for noise_from, divisor in ((1, 1.7), (0, 1.0)):
        got = capi.match_points_batch(ws, probs, divisor, cam, gs[0]["W"], 2.0, noise_from)
        for b, (q, pat) in enumerate(zip(probs, patterns)):
            want = capi.match_points(ws, q["flags"], q["raw_matched_loc1"], q["dpts0"], q["homo0"], divisor, q["dpt_map_1"], cam, gs[0]["W"],
                                     2.0, noise_from)
            assert got[b]["M"] == want["M"] == int(gs[b]["flags"].sum())
            assert np.float32(got[b]["mean_depth"]).tobytes() == np.float32(want["mean_depth"]).tobytes()
            for k in ("kept", "pts0", "pts1", "homo1", "dpts1", "noise_bounds"):
                a, w = got[b][k].cpu().numpy(), want[k].cpu().numpy()
                assert a.shape == w.shape and a.tobytes() == w.tobytes(), (b, pat, k, noise_from)
                rest = got[b]["full"][k][got[b]["M"]:]
                assert not rest.any().item(), (b, pat, k)            # nothing is written behind M (M = 0: nothing at all)
