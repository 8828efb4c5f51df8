"""Robust registration without a device: the fp64 restatement (tests/registration_ref.py) against the fixtures the
reference's own solver wrote (tests/golden/registration_*.npz, tests/golden/make_registration_golden.py), the conditions on
those fixtures the GPU tests rest on (no rounding difference can flip a discrete decision), and the host library
(sage_tls_estimate, sage_registration_finish) through the C ABI against the restatement.

Measured on the committed fixtures (largest over the 13 cases the reference solved; N = 2 apart, see below):
    restatement vs reference   |scale - ref| / scale = 0 (bit-equal in every case)   max |dR| 3.1e-14   max |dt| 4.7e-14
                               (both at n64_all_outliers, 15 GNC passes; bounds there 2.8e-7 / 2.1e-6)
    host library vs restatement   max |dR| 2.8e-14   max |dt| 4.1e-14 (same case)
    smallest margins   tied keys 0;  (second cost - lowest) / lowest 8.0e-7 (n1024);  pairs 5.5e-5 (n257);  translation
                       1.1e-3 (n512_o50);  GNC weights against 0.5: 1.3e-4 (n1024);  cost_diff against the threshold 0.11
At N = 2 the two chain TIMs are antiparallel: H has rank 1 and the rotation about that one direction is open -- Eigen's
JacobiSVD, LAPACK and the engine's Jacobi each pick their own.  What is determined is compared there: scale, every count and
mask, and that R maps the src TIM's direction onto the dst TIM's."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import capi, synth
from tests import registration_ref as ref

REFERENCE_CASES = [n for n, c in ref.CASES.items() if c["reference"]]
ALL_CASES = list(ref.CASES)


def test_fixtures_hold_the_synth_problems():
    """a fixture's inputs are what synth.make_registration_problem makes today (the generator and the tests see one problem)"""
    for name in ALL_CASES:
        fx, params = ref.load_case(name)
        prob = ref.make_case(name)
        for k in ("src", "dst", "noise_bounds"):
            assert fx[k].dtype == np.float32 and np.array_equal(fx[k], prob[k]), (name, k)
        assert params == prob["params"], name


@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_restatement_equals_the_reference(name):
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    n = fx["src"].shape[0]
    assert int(fx["ref_valid"]) == 1 and r["valid"]
    assert np.array_equal(r["inliers"], fx["ref_inliers"])
    assert np.array_equal(r["rotation_mask"], fx["ref_rotation_mask"])
    assert r["n_scale_inlier_pairs"] == int(fx["ref_n_scale_inlier_pairs"])
    d_scale = abs(r["scale"] - float(fx["ref_scale"])) / abs(r["scale"])
    assert d_scale <= r["bound"], (d_scale, r["bound"])          # both sums are sequential: the reorder bound is generous
    if np.isfinite(float(fx["ref_rotation_cost"])) or np.isfinite(r["rotation_cost"]):
        # the cost at termination tells the iteration the GNC left at (consecutive costs differ by >= the threshold)
        assert abs(r["rotation_cost"] - float(fx["ref_rotation_cost"])) < 0.5 * params["rotation_cost_threshold"]
    else:
        assert r["rotation_iterations"] == 0
    if n == 2:
        u_s = fx["src"][1].astype(np.float64) - fx["src"][0]; u_d = fx["dst"][1].astype(np.float64) - fx["dst"][0]
        for R in (r["R"], fx["ref_R"]):
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0
            assert np.allclose(R @ (u_s / np.linalg.norm(u_s)), u_d / np.linalg.norm(u_d), atol=1e-12)
        return
    b_R = ref.rotation_bound(r, n)
    b_t = ref.translation_bound(r, n, b_R, r["bound"])
    d_R = np.abs(r["R"] - fx["ref_R"]).max(); d_t = np.abs(r["t"] - fx["ref_t"]).max()
    print(f"{name}: |dscale|/scale {d_scale:.2e} (bound {r['bound']:.2e})  |dR| {d_R:.2e} (bound {b_R:.2e})  |dt| {d_t:.2e} (bound {b_t:.2e})")
    assert d_R <= b_R and d_t <= b_t


@pytest.mark.parametrize("name", ALL_CASES)
def test_fixture_conditions(name):
    """what lets a test demand exact lists from an evaluation that sums in another order"""
    r = ref.restated(name)
    v = r["vote"]
    assert v["ties"] == 0
    assert v["second_gap"] > 1e-9 * abs(v["cost"])
    assert r["pair_margin"] > 1e-6
    m = r["margins"]
    assert m["translation"] > 1e-6 and m["weight"] > 1e-6 and m["cost_diff"] > 1e-6 and m["mu"] > 1e-6
    assert m["translation_cost_gap"] > 1e-9


def test_cases_cover_what_they_are_meant_to():
    r = {n: ref.restated(n) for n in ALL_CASES}
    assert r["n2"]["n_pairs"] == 1 and r["n3"]["n_pairs"] == 3 and r["n1024"]["n_pairs"] == 523776
    assert r["n64_noise_free"]["rotation_iterations"] == 0 and r["n64_noise_free"]["n_inliers"] == 64
    assert r["n64_all_outliers"]["valid"] and r["n64_all_outliers"]["n_inliers"] < 8
    assert r["n64_coincident_src"]["n_degenerate_pairs"] == 8 and all(r[n]["n_degenerate_pairs"] == 0 for n in ALL_CASES if n != "n64_coincident_src")
    assert np.count_nonzero(r["n64_coincident_dst"]["X"] == 0.0) == 8
    assert np.all(ref.load_case("n64_clamp")[0]["noise_bounds"] == np.float32(5e-4))
    assert 0 < r["n512_o50"]["n_inliers"] <= 256 + 26 and r["n64_o0"]["n_inliers"] == 64
    assert any(0 < r[n]["rotation_iterations"] < 20 for n in ALL_CASES) and any(r[n]["rotation_iterations"] == 20 for n in ALL_CASES)


@pytest.mark.parametrize("name", ["n33", "n64_o30", "n512_o50"])
def test_scale_in_another_summation_order_stays_within_the_reorder_bound(name):
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    for block in (7, 64, 2048):
        rb = ref.scale_vote(fx["src"], fx["dst"], fx["noise_bounds"], params["cbar2"], block=block)
        assert rb["vote"]["min_index"] == r["vote"]["min_index"] and rb["n_scale_inlier_pairs"] == r["n_scale_inlier_pairs"]
        assert abs(rb["scale"] - r["scale"]) / r["scale"] <= r["bound"]


# ---- the host library through the C ABI (no device: they need the built library only)
def test_tls_estimate_is_the_sequential_vote():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 200):
        X = rng.normal(1.0, 0.2, n); X[: n // 3] += rng.normal(0, 2.0, n // 3)
        ranges = rng.uniform(0.01, 0.2, n)
        est, inl = capi.tls_estimate(X, ranges)
        v = ref.tls_estimate(X, ranges)
        assert est == v["estimate"] and np.array_equal(inl, v["inliers"]), n     # the same operations in the same order
    # the first of equal costs; a value alone is its own estimate
    est, inl = capi.tls_estimate(np.array([0.0, 10.0]), np.array([1.0, 1.0]))
    assert est == 0.0 and inl.tolist() == [True, False]
    est, inl = capi.tls_estimate(np.array([3.5]), np.array([0.25]))
    assert est == 3.5 and inl.tolist() == [True]


def test_tls_estimate_rejects_bad_arguments():
    x = np.ones(3)
    assert capi.tls_estimate_raw(None, x.ctypes.data, 3, None, None) == -1
    assert capi.tls_estimate_raw(x.ctypes.data, None, 3, None, None) == -1
    assert capi.tls_estimate_raw(x.ctypes.data, x.ctypes.data, 0, None, None) == -1
    assert capi.tls_estimate_raw(x.ctypes.data, x.ctypes.data, 3, None, None) == 0      # both outputs are optional


@pytest.mark.parametrize("name", ALL_CASES)
def test_host_finish_equals_the_restatement(name):
    fx, params = ref.load_case(name)
    r = ref.restated(name)
    n = fx["src"].shape[0]
    f = capi.registration_finish(fx["src"], fx["dst"], fx["noise_bounds"], r["scale"], params)
    assert f["valid"] == 1 and f["scale"] == r["scale"]
    assert np.array_equal(f["inliers"], r["inliers"]) and f["n_inliers"] == r["n_inliers"]
    assert np.array_equal(f["rotation_mask"], r["rotation_mask"]) and f["n_rotation_inliers"] == r["n_rotation_inliers"]
    assert f["rotation_iterations"] == r["rotation_iterations"]
    if n == 2:
        u_s = fx["src"][1].astype(np.float64) - fx["src"][0]; u_d = fx["dst"][1].astype(np.float64) - fx["dst"][0]
        assert np.allclose(f["R"] @ f["R"].T, np.eye(3), atol=1e-12) and np.linalg.det(f["R"]) > 0
        assert np.allclose(f["R"] @ (u_s / np.linalg.norm(u_s)), u_d / np.linalg.norm(u_d), atol=1e-12)
        return
    b_R = ref.rotation_bound(r, n)
    assert np.abs(f["R"] - r["R"]).max() <= b_R
    assert np.abs(f["t"] - r["t"]).max() <= ref.translation_bound(r, n, b_R, 0.0)


def test_host_finish_checks_its_arguments():
    fx, params = ref.load_case("n33")
    src, dst, nb = fx["src"], fx["dst"], fx["noise_bounds"]
    res = capi.SageRegistrationResult()
    p = capi.registration_params(params)
    args = lambda **kw: [kw.get("src", src.ctypes.data), kw.get("dst", dst.ctypes.data), kw.get("nb", nb.ctypes.data), kw.get("N", 33), 1.0,
                         kw.get("p", C.addressof(p)), kw.get("res", C.addressof(res)), None, None]
    assert capi.registration_finish_raw(*args()) == 0
    for bad in (dict(src=None), dict(dst=None), dict(nb=None), dict(p=None), dict(res=None), dict(N=1), dict(N=1025)):
        assert capi.registration_finish_raw(*args(**bad)) == -1, bad
    for field, value in (("rotation_tim_graph", capi.SAGE_REG_COMPLETE), ("inlier_selection_mode", capi.SAGE_REG_SELECT_PMC_EXACT),
                         ("inlier_selection_mode", capi.SAGE_REG_SELECT_KCORE_HEU), ("rotation_algorithm", capi.SAGE_REG_FGR)):
        q = capi.registration_params(params, **{field: value})
        assert capi.registration_finish_raw(*args(p=C.addressof(q))) == -2, field
    for field, value in (("cbar2", 0.0), ("noise_bound", -1.0), ("rotation_gnc_factor", 1.0), ("rotation_max_iterations", -1),
                         ("inlier_selection_mode", 4), ("rotation_tim_graph", 2), ("cbar2", float("nan"))):
        q = capi.registration_params(params, **{field: value})
        assert capi.registration_finish_raw(*args(p=C.addressof(q))) == -1, field


def test_registration_entry_points_check_their_arguments_before_touching_the_device():
    """NULL or out-of-range arguments and the unsupported modes are refused on the host: no workspace, no device needed"""
    p = capi.registration_params()
    res = capi.SageRegistrationResult()
    one = 8   # (a non-NULL pointer that is never followed: the workspace is NULL)
    assert capi.robust_registration_raw(None, one, one, one, 8, C.addressof(p), C.addressof(res), None, None) == -1
    cam = capi.SageCamera(100.0, 100.0, 32.0, 24.0, 64.0, 48.0)
    assert capi.match_points_raw(None, one, one, one, one, 1.0, one, C.addressof(cam), 8, 64, 2.0, 1, one, one, one, one, one, one,
                                 one, None) == -1


def test_synth_variants():
    for variant in synth.REG_VARIANTS:
        a = synth.make_registration_problem(40, 3, 0.25, 0.3, variant)
        b = synth.make_registration_problem(40, 3, 0.25, 0.3, variant)
        assert all(np.array_equal(a[k], b[k]) for k in ("src", "dst", "noise_bounds"))
        assert a["src"].dtype == np.float32 and a["src"].shape == (40, 3) and a["noise_bounds"].shape == (40,)
        assert np.all(a["noise_bounds"] >= np.float32(5e-4))
