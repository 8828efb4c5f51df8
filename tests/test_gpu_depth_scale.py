"""sage_depth_scale_ratio (Mapper::CorrectDepthScale / df::CorrectDepthScale on the device) against the fp64 restatement of
tests/depth_scale_ref.py.

Inputs: synth.make_depth_scale_problem at 48x64 (M = 2176: 9 workgroups; plain, zero patch, NaN texel, behind) and at 96x128
(M = 8708; "plain96" selects 8291 points, "big96" 1342).  The seeds are those at which the fp64 restatement finds no
ambiguous point (tests/test_depth_scale_ref.py::test_gpu_cases_have_no_ambiguous_point): counts and flags are exact.

Bounds.  Per point, a finite ratio may be off from fp64 by 8 x max(a, 2^-24) relative, where a is the largest relative distance
of the fp32 RESTATEMENT from the fp64 one over the points of that case, measured by the test on the CPU (the rule of
tests/test_gpu_track_overlap.py).  The median: an order statistic moves by no more than the largest per-point perturbation when
the selected sets are equal, so |ratio - ratio64| <= max_i |r_dev,i - r_64,i| over the selected finite points.

Measured, per case: a (CPU), the bound it gives, and what the device gave on an MI355X (largest relative distance from fp64):

  case         a        -> bound     device     |median - fp64| -> bound (largest per-point distance)
  plain        8.26e-7  -> 6.61e-6   8.26e-7    1.54e-7 -> 1.36e-6
  zero_patch   8.80e-6  -> 7.04e-5   8.80e-6    5.78e-9 -> 1.00e-4
  nan_texel    8.26e-7  -> 6.61e-6   8.26e-7    2.02e-8 -> 1.36e-6   (drop_nan = 1; NaN with drop_nan = 0)
  plain96      2.02e-6  -> 1.61e-5   2.02e-6    2.46e-7 -> 3.84e-6
  big96        9.14e-6  -> 7.32e-5   9.14e-6    5.22e-8 -> 1.46e-5
  behind       (no point has a finite non-zero ratio: nothing is selected, the others' ratios are 0 or NaN)

The device's distance equals the fp32 restatement's in every case: it rounds as the restatement does.  zero_patch and big96
are carried by points with a small D1 (next to the zero patch; at the image border, where taps fall outside)."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_scale_ref as ref
from tests.test_depth_scale_ref import CASES, case

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24


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


def dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(capi, ws, prob, drop_nan=False, gathered=True, per_point=True, **over):
    p = {**prob, **over}
    if gathered:
        dpt0, loc = dev(p["dpts0"]), None
    else:
        dpt0, loc = dev(p["dpt0_map"]), dev(p["loc1d0"], np.int64)
    r = capi.depth_scale_ratio(ws, p["R"], p["t"], dpt0, dev(p["homo"]), p["cam"], dev(p["bias1"]), dev(p["mask"]), p["eps"],
                               drop_nan, loc, per_point)
    if per_point:
        return r[0], r[1].cpu().numpy(), r[2].cpu().numpy()
    return r


def raw(st):
    return bytes(memoryview(st))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("drop_nan", [False, True])
def test_per_point_and_counts(capi, ws, name, drop_nan):
    """counts, flags, per-point ratios, the exactness of the selection and the median end to end; the measured figures are in
    the module's docstring"""
    prob, p64, p32, n_amb = case(name)
    st, ratios, selected = run(capi, ws, prob, drop_nan)
    s64 = ref.stats(prob, np.float64, drop_nan, p64)
    assert n_amb == 0
    print(f"{name} drop_nan {int(drop_nan)}: M {prob['M']} pos {st.n_pos_depth} selected {st.n_selected} nan {st.n_nan} used {st.n_used} "
          f"ratio {st.ratio!r} (fp64 {s64['ratio']!r})")
    # counts
    assert (st.n_points, st.n_pos_depth, st.n_selected, st.n_nan, st.n_used) == \
        (prob["M"], s64["n_pos_depth"], s64["n_selected"], s64["n_nan"], s64["n_used"])
    # per point
    assert np.array_equal(selected != 0, p64["selected"]) and set(np.unique(selected)) <= {0, 1}
    r64, r32 = p64["ratio"], p32["ratio"]
    fin = np.isfinite(r64) & (r64 != 0)
    assert np.array_equal(np.isnan(ratios), np.isnan(r64)) and np.array_equal(np.isinf(ratios), np.isinf(r64))
    assert np.array_equal(ratios[~fin & ~np.isnan(r64)], r64[~fin & ~np.isnan(r64)].astype(np.float32))   # zeros, infinities, their signs
    if fin.any():
        a = float(np.max(np.abs(r32[fin].astype(np.float64) - r64[fin]) / np.abs(r64[fin])))
        d = float(np.max(np.abs(ratios[fin].astype(np.float64) - r64[fin]) / np.abs(r64[fin])))
        print(f"    per point: fp32 restatement a {a:.2e} device {d:.2e} bound {8 * max(a, EPS24):.2e}")
        assert d <= 8 * max(a, EPS24)
    # the selection is exact: the lower median of the device's own per-point output
    want, n_used, n_nan = ref.lower_median(ratios[selected != 0], drop_nan)
    assert (n_used, n_nan) == (st.n_used, st.n_nan)
    assert (np.isnan(want) and np.isnan(st.ratio)) or np.float32(st.ratio) == want
    # end to end
    assert np.isnan(st.ratio) == np.isnan(s64["ratio"])
    if not np.isnan(s64["ratio"]):
        sf = p64["selected"] & np.isfinite(r64)
        worst = float(np.max(np.abs(ratios[sf].astype(np.float64) - r64[sf])))
        print(f"    median: |device - fp64| {abs(float(st.ratio) - s64['ratio']):.2e} bound {worst:.2e}")
        assert abs(float(st.ratio) - s64["ratio"]) <= worst


def test_modes(capi, ws):
    prob = case("nan_texel")[0]
    a, b = run(capi, ws, prob, False, per_point=False), run(capi, ws, prob, True, per_point=False)
    assert np.isnan(a.ratio) and a.n_nan > 0 and a.n_used == a.n_selected
    assert np.isfinite(b.ratio) and b.n_nan == a.n_nan and b.n_used == b.n_selected - b.n_nan
    st, ratios, selected = run(capi, ws, case("zero_patch")[0])
    assert np.isinf(ratios[selected != 0]).sum() > 0 and st.n_nan == 0 and st.n_used == st.n_selected and np.isfinite(st.ratio)
    for drop in (False, True):
        st = run(capi, ws, case("behind")[0], drop, per_point=False)          # returns: SAGE_OK
        assert st.n_selected == 0 and st.n_used == 0 and np.isnan(st.ratio) and 0 < st.n_pos_depth < st.n_points


@pytest.mark.parametrize("name", ["plain", "nan_texel", "plain96"])
def test_gathered_depths_and_map_with_locations_agree(capi, ws, name):
    prob = case(name)[0]
    a, b = run(capi, ws, prob, True, gathered=True), run(capi, ws, prob, True, gathered=False)
    assert raw(a[0]) == raw(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_a_location_outside_the_map_reads_nothing(capi, ws):
    """(the reference's index() throws) the point is not selected, the others are untouched"""
    prob = case("plain")[0]
    loc = prob["loc1d0"].copy()
    loc[[3, 1000]] = [-1, 48 * 64]
    st, ratios, selected = run(capi, ws, prob, gathered=False, loc1d0=loc)
    base, r0, s0 = run(capi, ws, prob)
    assert selected[3] == 0 and selected[1000] == 0 and st.n_selected == base.n_selected - int(s0[3]) - int(s0[1000])
    keep = np.ones(prob["M"], bool)
    keep[[3, 1000]] = False
    assert np.array_equal(ratios[keep], r0[keep]) and np.array_equal(selected[keep], s0[keep])


@pytest.mark.parametrize("name", ["plain", "plain96"])
def test_two_calls_return_the_same_bytes(capi, ws, name):
    prob = case(name)[0]
    a, b = run(capi, ws, prob), run(capi, ws, prob)
    assert raw(a[0]) == raw(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    w2 = capi.Workspace()
    try:
        c = run(capi, w2, prob)
    finally:
        w2.close()
    assert raw(a[0]) == raw(c[0]) and a[1].tobytes() == c[1].tobytes()


def test_workspace_grows_is_reused_and_shared_with_the_overlap_statistics(capi):
    """M = 300, the 48x64 case, 300 again on ONE workspace, a sage_track_overlap and a sage_median_f32 call in between: every
    result equals that of a workspace of its own"""
    from tests.test_gpu_track_overlap import case as ov_case, raw as ov_raw, run as ov_run
    prob = case("plain")[0]
    mid = prob["M"] // 2 - 150
    few = {**prob, "dpts0": prob["dpts0"][mid:mid + 300], "homo": prob["homo"][mid:mid + 300], "loc1d0": prob["loc1d0"][mid:mid + 300],
           "M": 300}
    ov_prob = ov_case("small")[0]
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)

    def fresh(call):
        w = capi.Workspace()
        try:
            return call(w)
        finally:
            w.close()

    want_ov = ov_raw(fresh(lambda w: ov_run(capi, w, ov_prob)))
    want_med = fresh(lambda w: capi.median_f32(w, dev(x)))
    one = capi.Workspace()
    try:
        for p in (few, prob, few):
            got, want = run(capi, one, p), fresh(lambda w: run(capi, w, p))
            print(f"M {p['M']}: selected {got[0].n_selected} ratio {got[0].ratio!r}")
            assert got[0].n_points == p["M"] and got[0].n_selected > 0 and np.isfinite(got[0].ratio)
            assert raw(got[0]) == raw(want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
            assert ov_raw(ov_run(capi, one, ov_prob)) == want_ov
            assert capi.median_f32(one, dev(x)) == want_med
    finally:
        one.close()


def test_misuse(capi, ws):
    """every SAGE_E_INVALID case returns at once (the output struct is untouched), and a valid call still works after them"""
    prob = case("plain")[0]
    R, t = np.ascontiguousarray(prob["R"], np.float32), np.ascontiguousarray(prob["t"], np.float32)
    bufs = dict(dpt0=dev(prob["dpts0"]), homo=dev(prob["homo"]), bias1=dev(prob["bias1"]), mask=dev(prob["mask"]))
    cam = prob["cam"]
    good_cam = dict(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, w=cam.w, h=cam.h)
    out = capi.SageDepthScaleStats()
    out.n_points = -7

    def call(ws_h=ws.h, R_=R.ctypes.data, t_=t.ctypes.data, dpt0=capi.dptr(bufs["dpt0"]), homo=capi.dptr(bufs["homo"]), M=prob["M"],
             camera=good_cam, bias1=capi.dptr(bufs["bias1"]), mask=capi.dptr(bufs["mask"]), out_=C.addressof(out)):
        c = capi.SageCamera(*[float(camera[k]) for k in ("fx", "fy", "cx", "cy", "w", "h")]) if camera is not None else None
        return capi.depth_scale_ratio_raw(ws_h, R_, t_, dpt0, None, homo, M, C.addressof(c) if c is not None else None, bias1, mask,
                                          float(prob["eps"]), 0, None, None, out_)

    bad = [dict(ws_h=None), dict(R_=None), dict(t_=None), dict(dpt0=None), dict(homo=None), dict(camera=None), dict(bias1=None),
           dict(mask=None), dict(out_=None), dict(M=0), dict(M=-5)]
    for k, v in (("fx", 0.0), ("fx", -1.0), ("fx", float("nan")), ("fx", float("inf")), ("fy", 0.0), ("fy", float("nan")),
                 ("fy", float("-inf")), ("w", 0.5), ("h", 0.0), ("w", float("nan"))):
        bad.append(dict(camera={**good_cam, k: v}))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert out.n_points == -7
    assert call() == 0
    assert raw(out) == raw(run(capi, ws, prob, per_point=False))
