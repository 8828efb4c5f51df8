"""The device finish's public calls without a device: the header declares them, the library exports them, the plan function
equals the formulas of include/sage_ba.h, and every argument check answers before anything touches the device.  The workspace
handle of these calls is a zeroed block of host memory, as in tests/test_registration_batch_api.py.

The formulas (SAGE_REG_FINISH_DEVICE; a problem with N >= 2 votes):
  launches       sage_robust_registration_batch_plan's + 1 (the finish kernel); 0 when nothing votes
  pinned bytes   Sum (64 + 32 N) [the votes' records] + Sum (128 + 8 N) [the finish's: R, t, counts | list | rotation mask]
  LDS bytes      49 840 per workgroup: 6 x 1024 doubles (the TIMs; later the translation's tile: 2048 x 12 bytes of endpoints
                 and 1024 x 16 of (X, r)) + 4 x (9 + 2 + 7) doubles of per-wave sums + 4 x 24 of minima + 4 x 4 of counts
  workgroups     the voting problems"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID, SAGE_E_UNSUPPORTED = -1, -2
LDS_BYTES = 6 * 1024 * 8 + 4 * (9 + 2 + 7) * 8 + 4 * 24 + 4 * 4
NEW = ("sage_workspace_set_registration_finish", "sage_workspace_registration_finish", "sage_registration_finish_batch",
       "sage_registration_finish_plan")


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"enum \{ SAGE_REG_FINISH_HOST = 0, SAGE_REG_FINISH_DEVICE = 1 \};", hdr)
    assert (capi.SAGE_REG_FINISH_HOST, capi.SAGE_REG_FINISH_DEVICE) == (0, 1)
    assert re.search(r"#define SAGE_REG_FINISH_MAX_ITERATIONS (\d+)", hdr).group(1) == str(capi.SAGE_REG_FINISH_MAX_ITERATIONS) == "1000"


PLAN_CASES = [(64,), (0, 257, 1), (91, 92), (2, 3, 33, 64, 257, 1024), (512, 257, 64, 5, 33, 3, 2, 1, 0), (0, 1, 1, 0), (512,) * 20,
              (1024,) * 32, ()]


@pytest.mark.parametrize("Ns", PLAN_CASES, ids=lambda t: "x".join(map(str, t[:9])) or "empty")
def test_plan_equals_the_formulas(Ns):
    got = capi.registration_finish_plan(Ns)
    vote = capi.robust_registration_batch_plan(Ns)
    voting = [n for n in Ns if n >= 2]
    want = dict(launches=vote["launches"] + 1 if voting else 0, pinned_bytes=sum(64 + 32 * n for n in voting) + sum(128 + 8 * n for n in voting),
                lds_bytes=LDS_BYTES if voting else 0, workgroups=len(voting))
    assert got == want
    assert got["pinned_bytes"] == vote["pinned_bytes"] + sum(128 + 8 * n for n in voting)
    if not voting:
        assert got == dict(launches=0, pinned_bytes=0, lds_bytes=0, workgroups=0)
    if Ns == (64,):
        assert got["launches"] == 1 + 2 + 2 + 6 + 1            # the single call's path (tests/test_registration_batch_api.py) + the finish
    if Ns == (512,) * 20:
        assert got["workgroups"] == 20 and got["lds_bytes"] == 49840 and got["pinned_bytes"] == 20 * (192 + 40 * 512)


def test_plan_checks_its_arguments_and_takes_null_outputs():
    n = np.array([64, 3], np.int32)
    raw = capi.registration_finish_plan_raw
    assert raw(n.ctypes.data, 2, None, None, None, None) == 0
    assert raw(None, 0, None, None, None, None) == 0
    assert raw(None, 2, None, None, None, None) == SAGE_E_INVALID
    assert raw(n.ctypes.data, -1, None, None, None, None) == SAGE_E_INVALID
    big = np.full(33, 8, np.int32)
    assert raw(big.ctypes.data, 33, None, None, None, None) == SAGE_E_INVALID
    for bad in (-1, 1025):
        m = np.array([64, bad], np.int32)
        assert raw(m.ctypes.data, 2, None, None, None, None) == SAGE_E_INVALID
    w = C.c_int32(-5)
    assert raw(n.ctypes.data, 2, None, None, None, C.addressof(w)) == 0 and w.value == 2


# ---- the mode and the argument checks of the calls that take a workspace
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
        self.rot = np.full((32, 16), 7, np.uint8)
        self.scales = np.ones(32)

    def probs(self, N, member=()):
        probs = (capi.SageRegistrationProblem * 32)(*[capi.SageRegistrationProblem(self.p, self.p, self.p, N[b] if b < len(N) else 8, 0.01,
                                                                                   None) for b in range(32)])
        for b, field, value in member:
            setattr(probs[b], field, value)
        return probs

    def finish(self, **kw):
        probs = self.probs(kw.pop("N", [8, 16, 5]), kw.pop("member", []))
        prm = capi.registration_params(kw.pop("params", None))
        a = dict(ws=C.addressof(self.ws), probs=C.addressof(probs), B=3, scales=self.scales.ctypes.data, p=C.addressof(prm),
                 res=C.addressof(self.res), inl=self.inl.ctypes.data, stride=16, rot=self.rot.ctypes.data)
        a.update(kw)
        return capi.registration_finish_batch_raw(a["ws"], a["probs"], a["B"], a["scales"], a["p"], a["res"], a["inl"], a["stride"], a["rot"])

    def batch(self, **kw):
        probs = self.probs(kw.pop("N", [8, 16, 5]))
        prm = capi.registration_params(kw.pop("params", None))
        return capi.robust_registration_batch_raw(C.addressof(self.ws), C.addressof(probs), 3, C.addressof(prm), C.addressof(self.res),
                                                  self.inl.ctypes.data, 16)

    def untouched(self):
        return all(r.valid == 77 for r in self.res) and bool((self.inl == -7).all()) and bool((self.rot == 7).all())


def test_mode_of_a_workspace():
    a = Args()
    ws = C.addressof(a.ws)
    get, put = capi.workspace_registration_finish_raw, capi.workspace_set_registration_finish_raw
    assert get(ws) == capi.SAGE_REG_FINISH_HOST and get(None) == capi.SAGE_REG_FINISH_HOST
    assert put(None, capi.SAGE_REG_FINISH_DEVICE) == SAGE_E_INVALID
    for mode in (-1, 2, 77):
        assert put(ws, mode) == SAGE_E_INVALID and get(ws) == capi.SAGE_REG_FINISH_HOST
    assert put(ws, capi.SAGE_REG_FINISH_DEVICE) == 0 and get(ws) == capi.SAGE_REG_FINISH_DEVICE
    assert put(ws, 2) == SAGE_E_INVALID and get(ws) == capi.SAGE_REG_FINISH_DEVICE
    assert put(ws, capi.SAGE_REG_FINISH_HOST) == 0 and get(ws) == capi.SAGE_REG_FINISH_HOST


FINISH_INVALID = [dict(ws=None), dict(probs=None), dict(scales=None), dict(p=None), dict(res=None), dict(B=-1), dict(B=33),
                  dict(N=[8, -1, 5]), dict(N=[8, 1025, 5]), dict(member=[(0, "src_dev", None)]), dict(member=[(1, "dst_dev", None)]),
                  dict(member=[(2, "noise_bounds_dev", None)]), dict(member=[(1, "noise_bound", 0.0)]),
                  dict(member=[(2, "noise_bound", float("inf"))]), dict(member=[(0, "noise_bound", float("nan"))]), dict(stride=15),
                  dict(stride=15, inl=None), dict(stride=15, rot=None), dict(params=dict(cbar2=0.0)),
                  dict(params=dict(rotation_max_iterations=-1)), dict(params=dict(rotation_gnc_factor=1.0)),
                  dict(params=dict(rotation_cost_threshold=float("inf"))), dict(params=dict(rotation_tim_graph=2)),
                  dict(params=dict(inlier_selection_mode=4)), dict(params=dict(rotation_algorithm=-1))]


@pytest.mark.parametrize("change", FINISH_INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_finish_batch_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.finish(**change) == SAGE_E_INVALID
    assert a.untouched()


@pytest.mark.parametrize("params", [dict(rotation_tim_graph=capi.SAGE_REG_COMPLETE), dict(inlier_selection_mode=capi.SAGE_REG_SELECT_PMC_EXACT),
                                    dict(rotation_algorithm=capi.SAGE_REG_FGR),
                                    dict(rotation_max_iterations=capi.SAGE_REG_FINISH_MAX_ITERATIONS + 1)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_finish_batch_answers_unsupported_without_a_device(params):
    a = Args()
    assert a.finish(params=params) == SAGE_E_UNSUPPORTED
    assert a.untouched()


def test_finish_batch_answers_empty_and_non_voting_batches_without_a_device():
    a = Args()
    assert a.finish(B=0) == 0 and a.untouched()
    assert a.finish(B=0, ws=None, probs=None, scales=None, p=None, res=None, inl=None, rot=None) == 0
    # rows with N < 2 take no part: none of their members is looked at, nothing is launched, the results are zeroed
    assert a.finish(N=[0, 1, 1], params=dict(noise_bound=0.0),
                    member=[(0, "src_dev", None), (1, "dst_dev", None), (2, "noise_bounds_dev", None), (1, "noise_bound", 0.0)]) == 0
    assert all(r.valid == 0 and r.n_inliers == 0 for r in a.res[:3]) and a.res[3].valid == 77
    assert (a.inl == -7).all() and (a.rot == 7).all()
    assert a.finish(N=[0, 1, 0], inl=None, rot=None, stride=0) == 0


def test_device_mode_refuses_an_iteration_cap_above_its_own_before_any_launch():
    """... and a batch in which nothing votes is answered in DEVICE mode as in HOST mode: no launch, the results zeroed"""
    a = Args()
    ws = C.addressof(a.ws)
    over = dict(rotation_max_iterations=capi.SAGE_REG_FINISH_MAX_ITERATIONS + 1)
    assert capi.workspace_set_registration_finish_raw(ws, capi.SAGE_REG_FINISH_DEVICE) == 0
    assert a.batch(params=over) == SAGE_E_UNSUPPORTED and a.untouched()
    one = capi.SageRegistrationResult(); one.valid = 77
    prm = capi.registration_params(over)
    assert capi.robust_registration_raw(ws, a.p, a.p, a.p, 8, C.addressof(prm), C.addressof(one), None, None) == SAGE_E_UNSUPPORTED
    assert one.valid == 77
    assert a.batch(N=[0, 1, 1]) == 0 and all(r.valid == 0 for r in a.res[:3]) and a.res[3].valid == 77
    f = capi.lib().sage_robust_registration_batch_launches
    f.argtypes = [C.c_void_p]
    assert f(ws) == 0
    # HOST mode takes the same cap (a batch in which nothing votes: the check is passed, nothing is launched)
    assert capi.workspace_set_registration_finish_raw(ws, capi.SAGE_REG_FINISH_HOST) == 0
    assert a.batch(N=[0, 1, 1], params=over) == 0
