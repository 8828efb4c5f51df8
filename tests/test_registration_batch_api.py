"""sage_robust_registration_batch, its plan and sage_match_points_batch without a device: the header declares them, the
library exports them, the plan function equals the formulas of include/sage_ba.h, and every argument check answers before
anything touches the device.  The workspace handle of these calls is a zeroed block of host memory, as in
tests/test_cycle_match_batch_api.py.

The formulas.  A problem with N >= 2 votes: pairs = N (N - 1) / 2, P = the power of two >= max(2 pairs, 4096).
  device bytes   Sum (12 P + 16 pairs + 160 (P / 2048) + 80)        pinned bytes   Sum (64 + 32 N)
  launches       those of sage_robust_registration for the largest problem alone, + 1 (the ticket's own launch) when two
                 or more problems vote (one voting problem takes the single call's path: no + 1):
                 1 + Sum over the powers of two 1024 < k <= P of (ceil((log2 k - 10) / 2) + 1) sort launches at the default
                 tile of 1024, + 6 (pairs, sums, offsets, cost, count, publish)
  order          descending P, rows of equal P in the caller's order, problems with N < 2 left out"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID, SAGE_E_UNSUPPORTED = -1, -2
BATCH_EXTRA_LAUNCHES = 1      # include/sage_ba.h: "+ 1 -- the ticket is a launch of its own", with two or more voting problems


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in ("sage_robust_registration_batch", "sage_robust_registration_batch_plan", "sage_robust_registration_batch_launches",
                 "sage_match_points_batch"):
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"#define SAGE_REG_MAX_BATCH (\d+)", hdr).group(1) == str(capi.SAGE_REG_MAX_BATCH) == "32"
    for struct, mirror in (("SageRegistrationProblem", capi.SageRegistrationProblem), ("SageMatchPointsItem", capi.SageMatchPointsItem)):
        body = re.search(r"typedef struct " + struct + r"[^{]*\{(.*?)\}\s*" + struct + ";", hdr, re.S)
        fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(capi.SageRegistrationProblem) == 48 and C.sizeof(capi.SageMatchPointsItem) == 88


# ---- the plan
def pairs_of(N):
    return N * (N - 1) // 2


def P_of(N):
    P = 4096
    while P < 2 * pairs_of(N):
        P *= 2
    return P


def single_launches(N):
    sort = 1 + sum(math.ceil((lk - 10) / 2) + 1 for lk in range(11, int(math.log2(P_of(N))) + 1))
    return sort + 6


def expected_plan(Ns):
    voting = [(b, n) for b, n in enumerate(Ns) if n >= 2]
    order = [b for b, n in sorted(voting, key=lambda bn: -P_of(bn[1]))]      # (sorted is stable)
    dev = sum(12 * P_of(n) + 16 * pairs_of(n) + 160 * (P_of(n) // 2048) + 80 for _, n in voting)
    pin = sum(64 + 32 * n for _, n in voting)
    launches = single_launches(max(n for _, n in voting)) + (BATCH_EXTRA_LAUNCHES if len(voting) > 1 else 0) if voting else 0
    return dict(device_bytes=dev, pinned_bytes=pin, launches=launches, order=order)


def test_the_formulas_at_known_sizes():
    assert [P_of(n) for n in (2, 46, 64, 91, 92, 512, 1024)] == [4096, 4096, 4096, 8192, 16384, 1 << 18, 1 << 20]
    assert pairs_of(46) == 1035 and pairs_of(512) == 130816
    assert single_launches(512) == 29 + 6 and single_launches(64) == 1 + 2 + 2 + 6 and single_launches(91) == 1 + 2 + 2 + 3 + 6


PLAN_CASES = [(64,), (0, 257, 1), (91, 92), (2, 3, 33, 64, 257, 1024), (46,) * 32, (0, 1, 1, 0), (1024, 0, 92, 1, 91, 92, 2, 512),
              (512,) * 20, (1024,) * 32, ()]


@pytest.mark.parametrize("Ns", PLAN_CASES, ids=lambda t: "x".join(map(str, t[:8])) or "empty")
def test_plan_equals_the_formulas(Ns):
    got = capi.robust_registration_batch_plan(Ns)
    want = expected_plan(Ns)
    assert got == want
    if Ns == (91, 92):
        assert got["order"] == [1, 0]                     # 92 has P = 16 384, 91 has 8 192
    if Ns == (2, 3, 33, 64, 257, 1024):
        assert got["order"] == [5, 4, 0, 1, 2, 3] and got["launches"] == single_launches(1024) + 1
    if Ns and max(Ns) < 2:
        assert got == dict(device_bytes=0, pinned_bytes=0, launches=0, order=[])


def test_plan_sizes_named_in_the_header():
    assert abs(capi.robust_registration_batch_plan((512,) * 20)["device_bytes"] - 105.2e6) < 0.1e6
    assert abs(capi.robust_registration_batch_plan((1024,) * 32)["device_bytes"] - 673.5e6) < 0.1e6


def test_plan_checks_its_arguments_and_takes_null_outputs():
    n = np.array([64, 3], np.int32)
    raw = capi.robust_registration_batch_plan_raw
    assert raw(n.ctypes.data, 2, None, None, None, None) == 0
    assert raw(None, 0, None, None, None, None) == 0
    assert raw(None, 2, None, None, None, None) == SAGE_E_INVALID
    assert raw(n.ctypes.data, -1, None, None, None, None) == SAGE_E_INVALID
    big = np.full(33, 8, np.int32)
    assert raw(big.ctypes.data, 33, None, None, None, None) == SAGE_E_INVALID
    for bad in (-1, 1025):
        m = np.array([64, bad], np.int32)
        assert raw(m.ctypes.data, 2, None, None, None, None) == SAGE_E_INVALID
    order = np.full(4, 9, np.int32)
    m = np.array([1, 64, 0, 92], np.int32)
    assert raw(m.ctypes.data, 4, None, None, None, order.ctypes.data) == 0 and order.tolist() == [3, 1, -1, -1]


# ---- the argument checks of the batch
class Args:
    """a valid argument set (B = 3) whose pointers are never followed: every case below changes one thing"""

    def __init__(self):
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        self.p = C.addressof(self.dummy)
        self.res = (capi.SageRegistrationResult * 32)()
        for r in self.res:
            r.valid = 77
        self.inl = np.full((32, 16), -7, np.int32)

    def batch(self, **kw):
        N = kw.pop("N", [8, 16, 5])
        probs = (capi.SageRegistrationProblem * 32)(*[capi.SageRegistrationProblem(self.p, self.p, self.p, N[b] if b < len(N) else 8, 0.01,
                                                                                   None) for b in range(32)])
        for b, field, value in kw.pop("member", []):
            setattr(probs[b], field, value)
        prm = capi.registration_params(kw.pop("params", None))
        a = dict(ws=C.addressof(self.ws), probs=C.addressof(probs), B=3, p=C.addressof(prm), res=C.addressof(self.res),
                 inl=self.inl.ctypes.data, stride=16)
        a.update(kw)
        return capi.robust_registration_batch_raw(a["ws"], a["probs"], a["B"], a["p"], a["res"], a["inl"], a["stride"])

    def untouched(self):
        return all(r.valid == 77 for r in self.res) and bool((self.inl == -7).all())


BATCH_INVALID = [dict(ws=None), dict(probs=None), dict(p=None), dict(res=None), dict(B=-1), dict(B=33), dict(N=[8, -1, 5]),
                 dict(N=[8, 1025, 5]), dict(member=[(0, "src_dev", None)]), dict(member=[(1, "dst_dev", None)]),
                 dict(member=[(2, "noise_bounds_dev", None)]), dict(member=[(1, "noise_bound", 0.0)]),
                 dict(member=[(1, "noise_bound", -1.0)]), dict(member=[(2, "noise_bound", float("inf"))]),
                 dict(member=[(0, "noise_bound", float("nan"))]), dict(stride=15), dict(params=dict(cbar2=0.0)),
                 dict(params=dict(cbar2=float("nan"))), dict(params=dict(rotation_max_iterations=-1)),
                 dict(params=dict(rotation_gnc_factor=1.0)), dict(params=dict(rotation_cost_threshold=float("inf"))),
                 dict(params=dict(rotation_tim_graph=2)), dict(params=dict(inlier_selection_mode=4)), dict(params=dict(rotation_algorithm=-1))]


@pytest.mark.parametrize("change", BATCH_INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_batch_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.batch(**change) == SAGE_E_INVALID
    assert a.untouched()


@pytest.mark.parametrize("field,value", [("rotation_tim_graph", capi.SAGE_REG_COMPLETE), ("inlier_selection_mode", capi.SAGE_REG_SELECT_PMC_EXACT),
                                         ("inlier_selection_mode", capi.SAGE_REG_SELECT_PMC_HEU),
                                         ("inlier_selection_mode", capi.SAGE_REG_SELECT_KCORE_HEU), ("rotation_algorithm", capi.SAGE_REG_FGR)])
def test_batch_answers_unsupported_modes_like_the_single_call(field, value):
    a = Args()
    assert a.batch(params={field: value}) == SAGE_E_UNSUPPORTED
    assert a.untouched()


def test_batch_answers_empty_and_non_voting_batches_without_a_device():
    a = Args()
    assert a.batch(B=0) == 0 and a.untouched()
    assert a.batch(B=0, ws=None, probs=None, p=None, res=None, inl=None) == 0
    # the caller's noise_bound is never read; a problem with N < 2 has none of its members looked at; inliers_host is optional
    assert a.batch(N=[0, 1, 1], params=dict(noise_bound=0.0),
                   member=[(0, "src_dev", None), (1, "dst_dev", None), (2, "noise_bounds_dev", None), (1, "noise_bound", 0.0)]) == 0
    assert all(r.valid == 0 and r.n_inliers == 0 and r.n_pairs == 0 for r in a.res[:3]) and a.res[3].valid == 77
    assert (a.inl == -7).all()
    assert a.batch(N=[0, 1, 0], inl=None, stride=0) == 0
    f = capi.lib().sage_robust_registration_batch_launches
    f.argtypes = [C.c_void_p]
    assert f(None) == 0 and f(C.addressof(a.ws)) == 0
    # the stride is compared with the largest N, voting or not
    assert a.batch(N=[0, 1, 0], stride=0) == SAGE_E_INVALID


# ---- the argument checks of the batched gather
def gather(**kw):
    ws = C.create_string_buffer(8192)
    dummy = C.create_string_buffer(64)
    p = C.addressof(dummy)
    items = (capi.SageMatchPointsItem * 32)(*[capi.SageMatchPointsItem(*([p] * 11)) for _ in range(32)])
    for b, field in kw.pop("null_member", []):
        setattr(items[b], field, None)
    cam = capi.SageCamera(60.0, 60.0, 3.5, 3.5, 8.0, 8.0)
    for k in ("fx", "fy"):
        if k in kw:
            setattr(cam, k, kw.pop(k))
    M = np.full(32, -3, np.int32)
    a = dict(ws=C.addressof(ws), items=C.addressof(items), B=3, cam=C.addressof(cam), K=5, W=8, nf=1, M=M.ctypes.data)
    a.update(kw)
    rc = capi.match_points_batch_raw(a["ws"], a["items"], a["B"], 1.0, a["cam"], a["K"], a["W"], 2.0, a["nf"], a["M"], None)
    assert (M == -3).all()
    return rc


GATHER_INVALID = [dict(ws=None), dict(items=None), dict(cam=None), dict(M=None), dict(B=-1), dict(B=33), dict(K=0), dict(W=0), dict(nf=2),
                  dict(nf=-1), dict(fx=0.0), dict(fy=float("nan")), dict(fx=float("inf"))] + \
                 [dict(null_member=[(b, f[0])]) for b, f in zip((0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1), capi.SageMatchPointsItem._fields_)]


@pytest.mark.parametrize("change", GATHER_INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_gather_batch_refuses_invalid_arguments_without_a_device(change):
    assert gather(**change) == SAGE_E_INVALID


def test_gather_batch_answers_an_empty_batch_with_ok():
    assert gather(B=0) == 0
    assert gather(B=0, ws=None, items=None, cam=None, M=None) == 0
