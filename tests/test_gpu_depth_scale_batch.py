"""sage_depth_scale_ratio_batch against sage_depth_scale_ratio, row by row and byte for byte: the statistics struct and both
per-point arrays, whatever the other rows, their order and their sizes; then the rows against the fp64 restatement.

A batch shares the keyframe to scale (bias, mask, camera), so the four 48x64 cases of tests/test_depth_scale_ref.py appear
here twice over: as the shared SIDE (the case's bias1 and mask: plain, with the zero patch, with the NaN texel, the constant
one of "behind") and as ROWS (a case's pose and point set):
  plain    the pose and the 2176 points of "plain" (= those of "zero_patch" and "nan_texel"): against the NaN-texel side it
           selects NaN ratios, against the zero-patch side +inf ratios
  top      the first 700 of those points, the upper rows of the image: it reaches neither the patch nor the NaN texel
  behind   the pose and points of "behind": selects nothing against any side, ratio NaN
A row whose side is its own case IS that case, and is compared with the fp64 restatement under the bound rule of
tests/test_gpu_depth_scale.py (per point 8 x max(a, 2^-24) with a measured on the CPU; the median within the largest
per-point distance); the figures measured there hold for it, since the row is byte-equal to the single call."""
import numpy as np
import pytest

from tests import depth_scale_ref as ref
from tests.test_depth_scale_ref import case

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
SIDES = ("plain", "zero_patch", "nan_texel", "behind")


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


@pytest.fixture(scope="module")
def data():
    """device copies, made once: per side (bias1, mask, cam, eps), per point set (R, t, gathered depths, map, locations, homo)"""
    sides, points = {}, {}
    for name in SIDES:
        p = case(name)[0]
        sides[name] = dict(bias1=dev(p["bias1"]), mask=dev(p["mask"]), cam=p["cam"], eps=p["eps"])
    for name in ("plain", "behind"):
        p = case(name)[0]
        points[name] = dict(R=p["R"], t=p["t"], dpts0=dev(p["dpts0"]), dmap=dev(p["dpt0_map"]), loc=dev(p["loc1d0"], np.int64),
                            homo=dev(p["homo"]), M=p["M"])
    return sides, points


def row(points="plain", M=None, gathered=True, per_point=True, off=0):
    """M points of a point set from its point `off` on (M None: all of them)"""
    return dict(points=points, M=M, gathered=gathered, per_point=per_point, off=off)


ROWS = dict(plain=row(), top=row(M=700), behind=row("behind"), plain_map=row(gathered=False))


def raw(st):
    return bytes(memoryview(st))


def single(capi, ws, data, side, r, drop_nan):
    """-> (the struct's bytes, the ratios' bytes, the flags' bytes) of sage_depth_scale_ratio on the row's inputs"""
    s, p = data[0][side], data[1][r["points"]]
    M, o = p["M"] if r["M"] is None else r["M"], r["off"]
    dpt0, loc = (p["dpts0"][o:o + M], None) if r["gathered"] else (p["dmap"], p["loc"][o:o + M])
    st, ratios, selected = capi.depth_scale_ratio(ws, p["R"], p["t"], dpt0, p["homo"][o:o + M], s["cam"], s["bias1"], s["mask"], s["eps"],
                                                  drop_nan, loc, True)
    return raw(st), ratios.cpu().numpy().tobytes(), selected.cpu().numpy().tobytes()


def batch(capi, ws, data, side, rows, drop_nan):
    """-> per row (the struct's bytes, the ratios' bytes or None, the flags' bytes or None), and the structs"""
    import torch
    s = data[0][side]
    crows, outs = [], []
    for r in rows:
        p = data[1][r["points"]]
        M, o = p["M"] if r["M"] is None else r["M"], r["off"]
        ratios = torch.full((M,), -7.0, dtype=torch.float32, device="cuda") if r["per_point"] else None
        selected = torch.full((M,), -7, dtype=torch.int32, device="cuda") if r["per_point"] else None
        outs.append((ratios, selected))
        if r["gathered"]:
            crows.append(capi.depth_scale_row(p["R"], p["t"], p["dpts0"][o:], p["homo"][o:], None, ratios, selected, M))
        else:
            crows.append(capi.depth_scale_row(p["R"], p["t"], p["dmap"], p["homo"][o:], p["loc"][o:], ratios, selected, M))
    stats = capi.depth_scale_ratio_batch(ws, crows, s["cam"], s["bias1"], s["mask"], s["eps"], drop_nan)
    got = [(raw(st), o[0].cpu().numpy().tobytes() if o[0] is not None else None, o[1].cpu().numpy().tobytes() if o[1] is not None else None)
           for st, o in zip(stats, outs)]
    return got, stats


def check(capi, ws, data, side, rows, drop_nan, want_ws=None):
    got, stats = batch(capi, ws, data, side, rows, drop_nan)
    assert len(got) == len(rows)
    for b, (g, r) in enumerate(zip(got, rows)):
        want = single(capi, want_ws or ws, data, side, r, drop_nan)
        assert g[0] == want[0], (side, b, r)
        if r["per_point"]:
            assert g[1] == want[1] and g[2] == want[2], (side, b, r)
    return stats


@pytest.mark.parametrize("drop_nan", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_one_row(capi, ws, data, side, drop_nan):
    for name in ("plain", "behind", "plain_map"):
        st = check(capi, ws, data, side, [ROWS[name]], drop_nan)[0]
        assert capi.depth_scale_ratio_batch_launches(ws) == capi.depth_scale_ratio_batch_plan([st.n_points])["launches"] == 5


@pytest.mark.parametrize("drop_nan", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_rows_side_by_side_in_both_orders(capi, ws, data, side, drop_nan):
    """the empty row's NaN and the rows with NaN or infinite ratios next to rows that have neither"""
    rows = [ROWS["plain"], ROWS["top"], ROWS["behind"], ROWS["plain_map"], ROWS["top"]]
    fwd = check(capi, ws, data, side, rows, drop_nan)
    rev = check(capi, ws, data, side, rows[::-1], drop_nan)
    assert [raw(s) for s in fwd] == [raw(s) for s in rev][::-1]
    plain, top, behind = fwd[0], fwd[1], fwd[2]
    print(f"{side} drop_nan {int(drop_nan)}: plain {plain.ratio!r} nan {plain.n_nan} used {plain.n_used}; top {top.ratio!r} used {top.n_used}; "
          f"behind {behind.ratio!r} selected {behind.n_selected}")
    assert behind.n_selected == 0 and np.isnan(behind.ratio)
    if side != "behind":
        assert top.n_nan == 0 and top.n_used > 0 and np.isfinite(top.ratio)          # untouched by its neighbours' NaNs
    if side == "nan_texel":
        assert plain.n_nan > 0 and np.isnan(plain.ratio) == (not drop_nan)


def test_thirty_two_rows(capi, ws, data):
    rows = [ROWS["plain"], ROWS["top"], ROWS["behind"], ROWS["plain_map"]] * 8
    for drop_nan in (False, True):
        stats = check(capi, ws, data, "nan_texel", rows, drop_nan)
        assert len(stats) == 32
        assert capi.depth_scale_ratio_batch_launches(ws) == capi.depth_scale_ratio_batch_plan([s.n_points for s in stats])["launches"] == 5


MIXED = (1, 2, 255, 256, 257, 2176)


@pytest.mark.parametrize("order", [MIXED, MIXED[::-1], (257, 1, 2176, 2, 256, 255)])
def test_mixed_sizes(capi, ws, data, order):
    """the problem's first M points: one point, two, a workgroup minus one point, exactly one, one plus a point, nine
    workgroups.  The very first points warp outside the mask, so the rows of 1 and 2 select nothing (NaN) next to rows that
    do; the rows of 255, 256 and 257 use 171, 172 and 173 ratios: odd and even counts (the LOWER median)"""
    rows = [row(M=m, gathered=(i % 2 == 0)) for i, m in enumerate(order)]
    for drop_nan in (False, True):
        stats = check(capi, ws, data, "plain", rows, drop_nan)
        assert [s.n_points for s in stats] == list(order)
        print(" ".join(f"M {s.n_points}: used {s.n_used} ratio {s.ratio!r}" for s in stats))
    by_m = {s.n_points: s for s in stats}
    assert by_m[2176].n_used > 0 and by_m[257].n_used > 0


def test_one_and_two_selected_points_next_to_larger_rows(capi, ws, data):
    """rows of one and of two points that the fp64 restatement selects (cut from the middle of the point set, where the warp
    lands inside the mask): the median of one key, the LOWER of two, next to rows of a workgroup and of nine"""
    sel = case("plain")[1]["selected"]
    mid = case("plain")[0]["M"] // 2
    off = next(i for i in range(mid, len(sel) - 1) if sel[i] and sel[i + 1])
    rows = [row(M=257), row(M=1, off=off), row(), row(M=2, off=off, gathered=False), row(M=2, off=off), row(M=1, off=off + 1, gathered=False)]
    for drop_nan in (False, True):
        stats = check(capi, ws, data, "plain", rows, drop_nan)
        assert [s.n_used for s in stats[1::2]] == [1, 2, 1] and stats[4].n_used == 2
        one, two, other = stats[1].ratio, stats[3].ratio, stats[5].ratio
        print(f"drop_nan {int(drop_nan)}: point {off}: {one!r}, point {off + 1}: {other!r}, the two: {two!r}")
        assert np.isfinite(one) and np.isfinite(other) and two == min(one, other) and stats[4].ratio == two


def test_the_scratch_grows_while_the_keys_do_not(capi, data):
    """a large single call first, then batches of more and more rows whose keys in all stay below it: the keys' allocation
    stays, the rows' scratch grows step by step, and every new row must start from zero -- every result equals that of a
    workspace that has seen nothing else"""
    sel = case("plain")[1]["selected"]
    mid = case("plain")[0]["M"] // 2
    steps = [[row(M=500, off=mid - 250 + 7 * b, gathered=(b % 2 == 0)) for b in range(4)],
             [row(M=250, off=mid - 125 + 11 * b) for b in range(8)],
             [row(M=60, off=mid - 30 + 3 * b, gathered=(b % 3 != 0)) for b in range(32)]]
    assert all(sum(r["M"] for r in rows) < 2176 for rows in steps)

    def fresh(call):
        w = capi.Workspace()
        try:
            return call(w)
        finally:
            w.close()

    want = [fresh(lambda w: batch(capi, w, data, "nan_texel", rows, True)[0]) for rows in steps]
    for first in (0, 1, 2):                       # the single call, then the batches from step `first` on
        one = capi.Workspace()
        try:
            single(capi, one, data, "nan_texel", ROWS["plain"], True)
            for rows, w in list(zip(steps, want))[first:]:
                got, stats = batch(capi, one, data, "nan_texel", rows, True)
                assert got == w, (first, len(rows))
                assert all(s.n_used > 0 for s in stats)
                assert single(capi, one, data, "nan_texel", ROWS["top"], True) == fresh(lambda v: single(capi, v, data, "nan_texel", ROWS["top"], True))
        finally:
            one.close()
    assert sel[mid]


def test_per_point_outputs_for_some_rows_only(capi, ws, data):
    rows = [row(), row(per_point=False), row(M=700, gathered=False), row("behind", per_point=False), row(M=257, per_point=False),
            row(M=300)]
    check(capi, ws, data, "zero_patch", rows, True)


def test_interleaved_with_the_single_calls_on_one_workspace(capi, data):
    """batch of 32, batch of 1, sage_depth_scale_ratio, sage_median_f32, the batch of 32 again on ONE workspace: every result
    equals that of a workspace that has seen nothing else"""
    big = [ROWS["plain"], ROWS["top"], ROWS["behind"], ROWS["plain_map"]] * 8
    x = dev(np.random.default_rng(3).standard_normal(1000).astype(np.float32))

    def fresh(call):
        w = capi.Workspace()
        try:
            return call(w)
        finally:
            w.close()

    want_big = fresh(lambda w: batch(capi, w, data, "nan_texel", big, True)[0])
    want_one = fresh(lambda w: batch(capi, w, data, "nan_texel", [ROWS["plain"]], True)[0])
    want_single = fresh(lambda w: single(capi, w, data, "nan_texel", ROWS["plain"], True))
    want_med = fresh(lambda w: capi.median_f32(w, x))
    want_meds = fresh(lambda w: capi.median_f32_batch(w, [x, x[:10]]))
    assert want_one[0] == want_single
    one = capi.Workspace()
    try:
        assert batch(capi, one, data, "nan_texel", big, True)[0] == want_big
        assert batch(capi, one, data, "nan_texel", [ROWS["plain"]], True)[0] == want_one
        assert capi.depth_scale_ratio_batch_launches(one) == 5
        assert single(capi, one, data, "nan_texel", ROWS["plain"], True) == want_single
        assert capi.median_f32(one, x) == want_med
        assert batch(capi, one, data, "nan_texel", big, True)[0] == want_big
        assert capi.depth_scale_ratio_batch_launches(one) == capi.depth_scale_ratio_batch_plan([2176, 700, 2176, 2176] * 8)["launches"]
        assert capi.median_f32_batch(one, [x, x[:10]]) == want_meds
        assert single(capi, one, data, "nan_texel", ROWS["top"], False) == fresh(lambda w: single(capi, w, data, "nan_texel", ROWS["top"], False))
    finally:
        one.close()


@pytest.mark.parametrize("drop_nan", [False, True])
@pytest.mark.parametrize("name", SIDES)
def test_rows_against_the_fp64_restatement(capi, ws, data, name, drop_nan):
    """row 0 is the case `name` itself, next to two other rows; the rule of tests/test_gpu_depth_scale.py"""
    prob, p64, p32, n_amb = case(name)
    own = ROWS["behind"] if name == "behind" else ROWS["plain"]
    got, stats = batch(capi, ws, data, name, [own, ROWS["top"], ROWS["behind"]], drop_nan)
    st = stats[0]
    ratios, selected = np.frombuffer(got[0][1], np.float32), np.frombuffer(got[0][2], np.int32)
    s64 = ref.stats(prob, np.float64, drop_nan, p64)
    assert n_amb == 0
    assert (st.n_points, st.n_pos_depth, st.n_selected, st.n_nan, st.n_used) == \
        (prob["M"], s64["n_pos_depth"], s64["n_selected"], s64["n_nan"], s64["n_used"])
    assert np.array_equal(selected != 0, p64["selected"]) and set(np.unique(selected)) <= {0, 1}
    r64, r32 = p64["ratio"], p32["ratio"]
    fin = np.isfinite(r64) & (r64 != 0)
    assert np.array_equal(np.isnan(ratios), np.isnan(r64)) and np.array_equal(np.isinf(ratios), np.isinf(r64))
    assert np.array_equal(ratios[~fin & ~np.isnan(r64)], r64[~fin & ~np.isnan(r64)].astype(np.float32))
    if fin.any():
        a = float(np.max(np.abs(r32[fin].astype(np.float64) - r64[fin]) / np.abs(r64[fin])))
        d = float(np.max(np.abs(ratios[fin].astype(np.float64) - r64[fin]) / np.abs(r64[fin])))
        print(f"{name} drop_nan {int(drop_nan)}: per point fp32 restatement a {a:.2e} device {d:.2e} bound {8 * max(a, EPS24):.2e}")
        assert d <= 8 * max(a, EPS24)
    want, n_used, n_nan = ref.lower_median(ratios[selected != 0], drop_nan)
    assert (n_used, n_nan) == (st.n_used, st.n_nan)
    assert (np.isnan(want) and np.isnan(st.ratio)) or np.float32(st.ratio) == want
    assert np.isnan(st.ratio) == np.isnan(s64["ratio"])
    if not np.isnan(s64["ratio"]):
        sf = p64["selected"] & np.isfinite(r64)
        worst = float(np.max(np.abs(ratios[sf].astype(np.float64) - r64[sf])))
        print(f"    median: |device - fp64| {abs(float(st.ratio) - s64['ratio']):.2e} bound {worst:.2e}")
        assert abs(float(st.ratio) - s64["ratio"]) <= worst
