"""The host rules of the partial relinearization (csrc/relin_plan.h behind sage_relin_plan and sage_relin_marks; no device
needed): which dense edges a changed group makes stale, which depth maps those edges read, and gtsam's relinearization check.

The reference of the plan is the reads table restated here edge by edge: a photometric edge a -> b reads pose a, pose b,
code a, scale a and the depth map of a; a geometric edge reads pose, code and scale of both and both depth maps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
POSE, CODE, SCALE = 1, 2, 4
NEW = ("sage_relin_plan", "sage_window_set_relinearization", "sage_window_last_evaluation", "sage_relin_marks",
       "sage_window_relin_marks", "sage_window_accept_marked")
K4_LINKS = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]       # a K = 4 chain with 2 back links: 10 directed edges per type


def values(K, CS, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((K, 12)).astype(np.float32), rng.standard_normal((K, CS)).astype(np.float32),
            (1.0 + rng.random(K)).astype(np.float32)]


def brute_plan(K, links, old, new):
    """the reads table, edge by edge: edge 2 l + d runs from the link's lower keyframe (d = 0) or to it (d = 1)"""
    differs = [[a[k].tobytes() != b[k].tobytes() for k in range(K)] for a, b in zip(old, new)]    # [pose, code, scale][k]
    dp, dc, ds = differs
    photo, geo, maps = [], [], np.zeros(K, np.uint8)
    for a, b in links:
        lo, hi = min(a, b), max(a, b)
        for src, dst in ((lo, hi), (hi, lo)):
            p = dp[src] or dp[dst] or dc[src] or ds[src]
            g = dp[src] or dp[dst] or dc[src] or dc[dst] or ds[src] or ds[dst]
            photo.append(int(p)); geo.append(int(g))
            if p or g:
                maps[src] = 1
            if g:
                maps[dst] = 1
    return np.array(photo, np.uint8), np.array(geo, np.uint8), maps


def check_plan(K, CS, links, old, new):
    got = capi.relin_plan(K, CS, links, old, new)
    photo, geo, maps = brute_plan(K, links, old, new)
    assert np.array_equal(got["photo_stale"], photo) and np.array_equal(got["geo_stale"], geo)
    assert np.array_equal(got["map_read"], maps)
    assert (got["n_photo"], got["n_geo"]) == (int(photo.sum()), int(geo.sum()))
    return got


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"SAGE_RELIN_ALL = 0, SAGE_RELIN_STALE = 1", hdr)
    assert (capi.SAGE_RELIN_ALL, capi.SAGE_RELIN_STALE) == (0, 1)
    assert C.sizeof(capi.SageEvalCounts) == 7 * 4 and C.sizeof(capi.SageRelinThresholds) == 8 * 4


# ----------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("CS", [16, 32])
def test_plan_one_group_of_one_keyframe_at_a_time(CS):
    K = 4
    old = values(K, CS)
    for k in range(K):
        for grp in range(3):
            new = [a.copy() for a in old]
            row = new[grp].reshape(K, -1)[k]                                              # (a view: the scales are [K])
            row[-1] = np.nextafter(row[-1], np.float32(9))                                # one element, one ulp
            got = check_plan(K, CS, K4_LINKS, old, new)
            touching = [e for e, (a, b) in enumerate((x for l in K4_LINKS for x in (l, l[::-1]))) if k in (a, b)]
            assert sorted(np.nonzero(got["geo_stale"])[0]) == touching                   # geometric: every edge touching k
            if grp == 0:
                assert np.array_equal(got["photo_stale"], got["geo_stale"])              # a pose: both types alike
            else:
                out_of_k = [e for e in touching if (K4_LINKS[e // 2] if e % 2 == 0 else K4_LINKS[e // 2][::-1])[0] == k]
                assert sorted(np.nonzero(got["photo_stale"])[0]) == out_of_k             # photometric: the edges OUT OF k only


def test_plan_code_of_keyframe_2():
    """the issue's example: photometric edges out of 2 and geometric edges touching 2 are stale, photometric edges into 2 clean"""
    K, CS = 4, 32
    old = values(K, CS, 1)
    new = [a.copy() for a in old]
    new[1][2, 5] += np.float32(0.25)
    got = check_plan(K, CS, K4_LINKS, old, new)
    directed = [x for l in K4_LINKS for x in (l, l[::-1])]
    for e, (src, dst) in enumerate(directed):
        assert got["photo_stale"][e] == (src == 2), (e, src, dst)
        assert got["geo_stale"][e] == (2 in (src, dst)), (e, src, dst)
    assert list(got["map_read"]) == [1, 1, 1, 1]                                         # 2 and its three neighbours


def test_plan_nothing_changed_and_signed_zero():
    K, CS = 4, 16
    old = values(K, CS, 2)
    old[1][3, 0] = np.float32(0.0)
    got = check_plan(K, CS, K4_LINKS, old, [a.copy() for a in old])
    assert not got["photo_stale"].any() and not got["geo_stale"].any() and not got["map_read"].any()
    assert (got["n_photo"], got["n_geo"]) == (0, 0)
    new = [a.copy() for a in old]
    new[1][3, 0] = np.float32(-0.0)                                                      # equal as floats, other bits
    assert new[1][3, 0] == old[1][3, 0]
    got = check_plan(K, CS, K4_LINKS, old, new)
    assert got["n_geo"] == 4 and got["n_photo"] == 2                                     # keyframe 3: links (1,3), (2,3)
    assert list(got["map_read"]) == [0, 1, 1, 1]


def test_plan_map_reads_follow_the_table():
    """a scale of an end keyframe: its out-edges' photometric factors read its own map only, the geometric ones both"""
    K, CS = 4, 16
    old = values(K, CS, 3)
    new = [a.copy() for a in old]
    new[2][0] *= np.float32(1.5)
    got = check_plan(K, CS, K4_LINKS, old, new)
    assert list(got["map_read"]) == [1, 1, 1, 0]
    # links given in either order of their keyframes number the same directed edges
    swapped = [(b, a) for a, b in K4_LINKS]
    again = capi.relin_plan(K, CS, swapped, old, new)
    assert all(np.array_equal(got[n], again[n]) for n in ("photo_stale", "geo_stale", "map_read"))
    # random links, several groups at once
    rng = np.random.default_rng(5)
    for trial in range(20):
        K = int(rng.integers(2, 9))
        links = [tuple(int(v) for v in rng.choice(K, 2, replace=False)) for _ in range(int(rng.integers(0, 12)))]
        old = values(K, CS, 10 + trial)
        new = [a.copy() for a in old]
        for _ in range(int(rng.integers(0, 4))):
            g, k = int(rng.integers(0, 3)), int(rng.integers(0, K))
            new[g][k].flat[0] += np.float32(1)
        check_plan(K, CS, links, old, new)


def test_plan_status_codes():
    K, CS = 4, 16
    v = values(K, CS)
    ptr = [a.ctypes.data for a in v]
    lk = np.asarray(K4_LINKS, np.int32)
    out = [np.zeros(10, np.uint8), np.zeros(10, np.uint8), np.zeros(K, np.uint8)]
    optr = [a.ctypes.data for a in out]

    def call(K_=K, CS_=CS, n=5, links=lk.ctypes.data, old=ptr, new=ptr, outs=optr):
        return capi.relin_plan_raw(K_, CS_, n, links, old, new, *outs, None, None)

    assert call() == OK                                                                  # (the counts are optional)
    for i in range(3):
        assert call(old=[p if j != i else None for j, p in enumerate(ptr)]) == INVALID
        assert call(new=[p if j != i else None for j, p in enumerate(ptr)]) == INVALID
        assert call(outs=[p if j != i else None for j, p in enumerate(optr)]) == INVALID
    assert call(links=None) == INVALID and call(n=0, links=None) == OK
    assert call(K_=0) == INVALID and call(CS_=0) == INVALID and call(n=-1) == INVALID
    for bad in ([(0, 4)], [(-1, 2)], [(2, 2)]):
        b = np.asarray(bad, np.int32)
        assert call(n=1, links=b.ctypes.data) == INVALID


# ---------------------------------------------------------------------------------------------------------------- the marks
@pytest.mark.parametrize("CS", [16, 32])
def test_marks_are_strict_and_per_group(CS):
    t = capi.relin_thresholds(pose=[1e-3, 2e-3, 3e-3, 4e-3, 5e-3, 6e-3], code=1e-4, scale=1e-3)
    B = 7 + CS
    thr = np.array(list(t.pose) + [t.code] * CS + [t.scale], np.float64)                # (the fp32 thresholds, widened)
    K = 3
    d = np.zeros((K, B))
    d[:] = thr                                                                           # equal to the threshold: nothing
    d[1] *= -1
    marks, n = capi.relin_marks(d, K, CS, t)
    assert list(marks) == [0, 0, 0] and n == 0
    up = np.nextafter(thr, np.inf)
    for row, want in ((3, POSE), (6 + CS - 1, CODE), (6, CODE), (6 + CS, SCALE)):        # one element over: its group only
        for sign in (1.0, -1.0):
            d = np.zeros((K, B)); d[:] = thr
            d[2, row] = sign * up[row]
            marks, n = capi.relin_marks(d, K, CS, t)
            assert list(marks) == [0, 0, want] and n == 1
    d = np.zeros((K, B))
    d[0, 0] = 1.0; d[0, 6 + CS] = -1.0; d[1, 7] = 1.0                                    # groups independently
    marks, n = capi.relin_marks(d, K, CS, t)
    assert list(marks) == [POSE | SCALE, CODE, 0] and n == 3
    d = np.full((K, B), np.nan)                                                          # a NaN marks nothing
    marks, n = capi.relin_marks(d, K, CS, t)
    assert list(marks) == [0, 0, 0] and n == 0
    d[1, 2] = np.inf
    assert list(capi.relin_marks(d, K, CS, t)[0]) == [0, POSE, 0]
    d1 = np.zeros((1, B)); d1[0, 6 + CS] = 2e-3                                          # K = 1
    marks, n = capi.relin_marks(d1, 1, CS, t)
    assert list(marks) == [SCALE] and n == 1
    t2 = capi.relin_thresholds()                                                         # the mapper's thresholds
    assert [round(float(v), 9) for v in t2.pose] == [0.001] * 6 and (round(t2.code, 9), round(t2.scale, 9)) == (0.0001, 0.001)


def test_marks_and_window_calls_status_codes():
    t = capi.relin_thresholds()
    d = np.zeros(23); m = np.zeros(1, np.int32)
    tp = C.addressof(t)
    assert capi.relin_marks_raw(d.ctypes.data, 1, 16, tp, m.ctypes.data, None) == OK
    assert capi.relin_marks_raw(None, 1, 16, tp, m.ctypes.data, None) == INVALID
    assert capi.relin_marks_raw(d.ctypes.data, 1, 16, None, m.ctypes.data, None) == INVALID
    assert capi.relin_marks_raw(d.ctypes.data, 1, 16, tp, None, None) == INVALID
    assert capi.relin_marks_raw(d.ctypes.data, 0, 16, tp, m.ctypes.data, None) == INVALID
    assert capi.relin_marks_raw(d.ctypes.data, 1, 0, tp, m.ctypes.data, None) == INVALID
    L = capi.lib()
    n = capi.SageEvalCounts()
    for mode in (capi.SAGE_RELIN_ALL, capi.SAGE_RELIN_STALE, 2, -1):
        assert L.sage_window_set_relinearization(None, mode) == INVALID
    assert L.sage_window_last_evaluation(None, C.byref(n)) == INVALID
    assert L.sage_window_relin_marks(None, C.byref(t), m.ctypes.data_as(C.POINTER(C.c_int32)), None) == INVALID
    assert L.sage_window_accept_marked(None, m.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
