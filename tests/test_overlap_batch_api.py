"""sage_track_overlap_batch, its plan and its launch count without a device: the header declares them, the library exports
them, the plan function equals the formulas of include/sage_ba.h, and every argument check answers before anything touches
the device.  The workspace handle of these calls is a zeroed block of host memory, as in tests/test_registration_batch_api.py.

The formulas, for B >= 1 poses over M points (0 for B = 0):
  workgroups per row   min(ceil(M / 256), 32): sage_track_overlap's partition
  pinned bytes         32 B + 8 M (B + 1): a header per row, the input set once, a warped set per row
  device bytes         12816 B + 8 M (B + 1): per row 32 partial records of 8 + 8 + 384 bytes and 16 bytes of counters
  launches             3"""
import ctypes as C
import os
import re

import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_E_INVALID = -1
NAMES = ("sage_track_overlap_batch", "sage_track_overlap_batch_plan", "sage_track_overlap_batch_launches")


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"#define SAGE_OVERLAP_MAX_BATCH (\d+)", hdr).group(1) == str(capi.OVERLAP_MAX_BATCH) == "32"
    assert re.search(r"#define SAGE_TRACK_MAX_BATCH (\d+)", hdr).group(1) == "32"
    body = re.search(r"typedef struct SageOverlapPose[^{]*\{(.*?)\}\s*SageOverlapPose;", hdr, re.S)
    fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    assert fields == [f[0] for f in capi.SageOverlapPose._fields_]
    assert C.sizeof(capi.SageOverlapPose) == 13 * 4


@pytest.mark.parametrize("B", [1, 2, 32])
def test_plan_launches_three_whatever_B(B):
    assert capi.track_overlap_batch_plan(2176, B)["launches"] == 3


def test_plan_of_an_empty_batch():
    assert capi.track_overlap_batch_plan(2176, 0) == dict(device_bytes=0, pinned_bytes=0, launches=0, workgroups_per_row=9)
    assert capi.track_overlap_batch_plan(0, 0)["launches"] == 0


@pytest.mark.parametrize("M,want", [(1, 1), (256, 1), (257, 2), (8192, 32), (8193, 32)])
def test_plan_keeps_the_single_calls_partition(M, want):
    for B in (1, 32):
        assert capi.track_overlap_batch_plan(M, B)["workgroups_per_row"] == want


@pytest.mark.parametrize("M", [1, 257, 2176, 58052])
def test_plan_bytes(M):
    last = 0
    for B in range(1, 33):
        p = capi.track_overlap_batch_plan(M, B)
        assert p["pinned_bytes"] == B * 32 + 8 * M * (B + 1)
        assert p["device_bytes"] == 12816 * B + 8 * M * (B + 1)          # (the header's formula)
        assert p["device_bytes"] >= 8 * M * (B + 1) and p["device_bytes"] >= last
        last = p["device_bytes"]


def test_plan_checks_its_arguments_and_takes_null_outputs():
    raw = capi.track_overlap_batch_plan_raw
    assert raw(2176, 3, None, None, None, None) == 0
    assert raw(2176, 0, None, None, None, None) == 0
    launches = C.c_int32(77)
    assert raw(2176, 32, None, None, C.addressof(launches), None) == 0 and launches.value == 3
    for M, B in ((2176, -1), (2176, 33), (0, 1), (-5, 2)):
        launches.value = 77
        assert raw(M, B, None, None, C.addressof(launches), None) == SAGE_E_INVALID and launches.value == 77


class Args:
    """a valid argument set (B = 3) whose pointers are never followed: every case below changes one thing"""

    def __init__(self):
        self.ws = C.create_string_buffer(8192)
        self.dummy = C.create_string_buffer(64)
        self.p = C.addressof(self.dummy)
        self.poses = (capi.SageOverlapPose * 33)()
        self.cam = capi.SageCamera(57.6, 57.6, 31.5, 23.5, 64.0, 48.0)
        self.out = (capi.SageOverlapStats * 33)()
        for o in self.out:
            o.n_points = 77

    def batch(self, **kw):
        for k, v in kw.pop("cam_fields", {}).items():
            setattr(self.cam, k, v)
        a = dict(ws=C.addressof(self.ws), poses=C.addressof(self.poses), B=3, dpts0=self.p, homo=self.p, M=100,
                 cam=C.addressof(self.cam), mask=self.p, eps=1e-4, out=C.addressof(self.out))
        a.update(kw)
        return capi.track_overlap_batch_raw(a["ws"], a["poses"], a["B"], a["dpts0"], a["homo"], a["M"], a["cam"], a["mask"], a["eps"],
                                            a["out"])

    def untouched(self):
        return all(o.n_points == 77 for o in self.out)


INVALID = [dict(ws=None), dict(B=-1), dict(B=33), dict(poses=None), dict(dpts0=None), dict(homo=None), dict(cam=None), dict(mask=None),
           dict(out=None), dict(M=0), dict(M=-3), dict(cam_fields=dict(fx=0.0)), dict(cam_fields=dict(fy=-1.0)),
           dict(cam_fields=dict(fx=float("nan"))), dict(cam_fields=dict(fy=float("inf"))), dict(cam_fields=dict(w=0.5)),
           dict(cam_fields=dict(h=0.0)), dict(cam_fields=dict(w=32769.0)), dict(cam_fields=dict(h=float("inf")))]


@pytest.mark.parametrize("change", INVALID, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_batch_refuses_invalid_arguments_without_a_device(change):
    a = Args()
    assert a.batch(**change) == SAGE_E_INVALID
    assert a.untouched()


def test_the_single_call_refuses_the_same_cameras():
    """'the camera checks of sage_track_overlap with the same bounds'"""
    for change in INVALID:
        if "cam_fields" not in change:
            continue
        a = Args()
        for k, v in change["cam_fields"].items():
            setattr(a.cam, k, v)
        out = capi.SageOverlapStats()
        assert capi.track_overlap_raw(C.addressof(a.ws), a.p, a.p, a.p, 1.0, a.p, 100, C.addressof(a.cam), a.p, 1e-4,
                                      C.addressof(out)) == SAGE_E_INVALID, change


def test_an_empty_batch_reads_nothing_and_needs_no_device():
    a = Args()
    assert a.batch(B=0) == 0 and a.untouched()
    assert a.batch(B=0, poses=None, dpts0=None, homo=None, cam=None, mask=None, out=None, M=0) == 0 and a.untouched()
    f = capi.lib().sage_track_overlap_batch_launches
    f.argtypes = [C.c_void_p]
    assert f(None) == 0 and f(C.addressof(a.ws)) == 0
    assert capi.track_overlap_batch_launches(None) == 0
