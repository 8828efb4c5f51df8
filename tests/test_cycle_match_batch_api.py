"""sage_cycle_match_batch and sage_loop_precheck without a device: the header declares them, the library exports them, and
every argument check answers before anything touches the device.  The workspace handle of these calls is a zeroed block of
host memory: validation, and the B = 0 / K = 0 answers, must not read it (NULL is refused, so the checks behind the first
one can only be reached with a handle)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID, SAGE_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def hdr():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        return fh.read()


def test_header_declares_and_library_exports(hdr):
    L = capi.lib()
    for name in ("sage_cycle_match_batch", "sage_cycle_match_batch_slices", "sage_loop_precheck"):
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"#define SAGE_MATCH_MAX_BATCH (\d+)", hdr).group(1) == str(capi.SAGE_MATCH_MAX_BATCH) == "32"
    assert "typedef struct SageLoopCandidate" in hdr and "typedef struct SageLoopPrecheckResult" in hdr
    assert "#define SAGE_E_INVALID (-1)" in hdr and "#define SAGE_E_UNSUPPORTED (-2)" in hdr


class Args:
    """a valid argument set (B = 3, K = 5) whose pointers are never followed: every case below changes one thing"""

    def __init__(self):
        self.ws = C.create_string_buffer(4096)
        self.dummy = C.create_string_buffer(64)
        p = C.addressof(self.dummy)
        self.B, self.K = 3, 5
        self.cand = (C.c_void_p * 32)(*([p] * 32))
        self.kp = (C.c_void_p * 32)(*([p] * 32))
        self.counts = np.full(32, -1, np.int32)
        self.p = p

    def batch(self, **kw):
        a = dict(ws=C.addressof(self.ws), q=self.p, cand=C.addressof(self.cand), kp=C.addressof(self.kp), B=self.B, K=self.K, C=16, H=8,
                 W=8, slices=0, raw=self.p, cyc=self.p, flags=self.p, counts=self.counts.ctypes.data)
        a.update(kw)
        return capi.cycle_match_batch_raw(a["ws"], a["q"], a["cand"], a["kp"], a["B"], a["K"], a["C"], a["H"], a["W"], 1.0, a["slices"],
                                          a["raw"], a["cyc"], a["flags"], a["counts"])

    def precheck(self, **kw):
        cands = (capi.SageLoopCandidate * 32)(*[capi.SageLoopCandidate(self.p, self.p, self.p, self.p, self.p) for _ in range(32)])
        for b, field in kw.pop("null_member", []):
            setattr(cands[b], field, None)
        cam = capi.SageCamera(60.0, 60.0, 3.5, 3.5, 8.0, 8.0)
        for k in ("fx", "fy"):
            if k in kw:
                setattr(cam, k, kw.pop(k))
        prm = capi.registration_params(kw.pop("params", None))
        self.results = (capi.SageLoopPrecheckResult * 32)()
        for r in self.results:
            r.n_cycle = 77
        a = dict(ws=C.addressof(self.ws), q=self.p, cands=C.addressof(cands), B=self.B, K=self.K, C=16, H=8, W=8, cam=C.addressof(cam),
                 p=C.addressof(prm), results=C.addressof(self.results), raw=self.p, flags=self.p, ikp=self.p)
        a.update(kw)
        return capi.loop_precheck_raw(a["ws"], a["q"], 1.0, a["cands"], a["B"], a["K"], a["C"], a["H"], a["W"], a["cam"], 1.0, 2.0, 0.3,
                                      a["p"], a["results"], a["raw"], a["flags"], a["ikp"])


BATCH_INVALID = [dict(ws=None), dict(B=33), dict(B=-1), dict(K=-1), dict(C=0), dict(C=1025), dict(H=0), dict(W=0), dict(slices=-1),
                 dict(counts=None), dict(q=None), dict(cand=None), dict(kp=None), dict(raw=None), dict(cyc=None), dict(flags=None)]


@pytest.mark.parametrize("change", BATCH_INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_batch_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.batch(**change) == SAGE_E_INVALID
    assert (a.counts == -1).all()                       # nothing was written either


@pytest.mark.parametrize("which,b", [("cand", 0), ("cand", 2), ("kp", 1)])
def test_batch_refuses_a_null_entry_of_a_pointer_array(which, b):
    a = Args()
    getattr(a, which)[b] = None
    assert a.batch() == SAGE_E_INVALID
    getattr(a, which)[b] = a.p
    getattr(a, which)[3] = None                          # (an entry past B is not looked at)
    assert a.batch(K=0) == 0


def test_batch_answers_empty_calls_with_ok_and_zero_counts():
    a = Args()
    assert a.batch(B=0) == 0 and (a.counts == -1).all()
    assert a.batch(B=0, cand=None, kp=None, counts=None, q=None, raw=None, cyc=None, flags=None) == 0
    assert a.batch(K=0) == 0
    assert (a.counts[:3] == 0).all() and (a.counts[3:] == -1).all()
    assert a.batch(K=0, cand=None, kp=None, q=None, raw=None, cyc=None, flags=None) == 0
    assert a.batch(K=0, slices=10 ** 6) == 0
    f = capi.lib().sage_cycle_match_batch_slices
    f.argtypes = [C.c_void_p]
    assert f(None) == 0 and f(C.addressof(a.ws)) == 0


PRECHECK_INVALID = [dict(ws=None), dict(cands=None), dict(cam=None), dict(p=None), dict(results=None), dict(B=33), dict(B=-1), dict(K=-1),
                    dict(K=1025), dict(C=0), dict(C=1025), dict(H=0), dict(W=0), dict(q=None), dict(raw=None), dict(flags=None),
                    dict(ikp=None), dict(null_member=[(1, "desc_dev")]), dict(null_member=[(2, "dpt_map_dev")]),
                    dict(null_member=[(0, "kp_loc1d_dev")]), dict(null_member=[(0, "kp_dpts0_dev")]), dict(null_member=[(2, "kp_homo0_dev")]),
                    dict(fx=0.0), dict(fy=float("nan")), dict(params=dict(cbar2=0.0)), dict(params=dict(rotation_max_iterations=-1))]


@pytest.mark.parametrize("change", PRECHECK_INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_precheck_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.precheck(**change) == SAGE_E_INVALID
    assert all(r.n_cycle == 77 for r in a.results)


def test_precheck_answers_unsupported_modes_like_the_registration():
    a = Args()
    assert a.precheck(params=dict(rotation_tim_graph=capi.SAGE_REG_COMPLETE)) == SAGE_E_UNSUPPORTED
    assert all(r.n_cycle == 77 for r in a.results)


def test_precheck_answers_empty_calls_with_ok_and_zeroed_results():
    a = Args()
    assert a.precheck(B=0) == 0 and all(r.n_cycle == 77 for r in a.results)
    assert a.precheck(K=0) == 0
    assert all(r.n_cycle == 0 and r.registered == 0 and r.n_matched == 0 for r in a.results[:3]) and a.results[3].n_cycle == 77
    assert a.precheck(K=0, params=dict(noise_bound=0.0)) == 0      # (the caller's noise_bound is never read)
