"""Prepared keyframes, the host half (no device): the plan of a prepare call, the configuration fingerprint a window compares
before it takes a handle, and the statuses of NULL / 0 arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NEW = ["sage_keyframe_prepare", "sage_keyframe_prepare_batch", "sage_keyframe_prepare_plan", "sage_keyframe_prepare_launches",
       "sage_keyframe_config_matches", "sage_keyframe_info", "sage_keyframe_get", "sage_window_add_prepared_keyframe",
       "sage_window_build_stats"]
ALIGN = 256            # every sub-array of a handle's allocation starts at a multiple of it
SUBARRAYS = 4          # planes | locations | rays | pre-sampled features


def config(H, W, L=2, FS=16, CS=32) -> capi.SageWindowConfig:
    cfg = capi.SageWindowConfig()
    cfg.pyr = capi.make_pyramid(synth.Camera(0.9 * W, 0.9 * W, W / 2.0, H / 2.0, W, H), L)
    cfg.FS, cfg.CS = FS, CS
    for l in range(L):
        cfg.photo_weights[l] = 10.0 - l
    return cfg


def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int\s+" + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"^void sage_keyframe_release\(", hdr, re.M) and "sage_keyframe_release" in capi.SYMBOLS
    assert re.search(r"#define SAGE_PREPARE_MAX_BATCH 64\b", hdr) and capi.SAGE_PREPARE_MAX_BATCH == 64
    assert re.search(r"SAGE_PREP_PACKED = 0, SAGE_PREP_LOC = 1, SAGE_PREP_HOMO = 2, SAGE_PREP_F0S = 3", hdr)
    assert (capi.SAGE_PREP_PACKED, capi.SAGE_PREP_LOC, capi.SAGE_PREP_HOMO, capi.SAGE_PREP_F0S) == (0, 1, 2, 3)
    assert C.sizeof(capi.SagePreparedInfo) == 5 * 4 + 4 + 8 and C.sizeof(capi.SageWindowBuildStats) == 6 * 4


@pytest.mark.parametrize("H,W", [(32, 48), (38, 62)])
def test_plan_sizes_a_handle_from_its_samples(H, W):
    cfg = config(H, W)
    FS, L, P = cfg.FS, cfg.pyr.levels, cfg.pyr.P
    N = [512, 200, 1, 1012]
    plan = capi.keyframe_prepare_plan(cfg, N)
    for n, got in zip(N, plan["device_bytes"]):
        cap = max(1, -(-5 * n // 4))
        floor = 12 * FS * P + cap * (8 + 12 + 4 * L * FS)
        assert floor <= got <= floor + SUBARRAYS * ALIGN, (n, got, floor)
    # the sparse keyframe: far below a whole image of tiles with all 64 slots, which is what a window's own copy reserves
    tiles = ((W + 7) // 8) * ((H + 7) // 8) * 64
    assert plan["device_bytes"][1] < 12 * FS * P + tiles * (8 + 12 + 4 * L * FS)
    assert plan["scratch_bytes"] >= len(N) * H * W * 4
    for B in (1, 2, 7, 64):
        p = capi.keyframe_prepare_plan(cfg, [300] * B)
        assert (p["launches"], p["waits"]) == (6, 2) and p["scratch_bytes"] >= B * H * W * 4
        assert p["device_bytes"] == [p["device_bytes"][0]] * B


def test_plan_refuses_what_prepare_refuses():
    cfg = config(32, 48)
    n = np.array([10, 20], np.int32)
    for B in (0, -1, 65):
        assert capi.keyframe_prepare_plan_raw(C.byref(cfg), n.ctypes.data, B, None, None, None, None) == INVALID
    assert capi.keyframe_prepare_plan_raw(None, n.ctypes.data, 2, None, None, None, None) == INVALID
    assert capi.keyframe_prepare_plan_raw(C.byref(cfg), None, 2, None, None, None, None) == INVALID
    assert capi.keyframe_prepare_plan_raw(C.byref(cfg), n.ctypes.data, 2, None, None, None, None) == 0   # outputs: optional
    neg = np.array([10, -1], np.int32)
    assert capi.keyframe_prepare_plan_raw(C.byref(cfg), neg.ctypes.data, 2, None, None, None, None) == INVALID
    for FS in (0, 18):
        bad = capi.SageWindowConfig.from_buffer_copy(cfg); bad.FS = FS
        assert capi.keyframe_prepare_plan_raw(C.byref(bad), n.ctypes.data, 2, None, None, None, None) == INVALID
    for wgt in (-1.0, float("nan")):
        bad = capi.SageWindowConfig.from_buffer_copy(cfg); bad.photo_weights[1] = wgt
        assert capi.keyframe_prepare_plan_raw(C.byref(bad), n.ctypes.data, 2, None, None, None, None) == INVALID
    bad = capi.SageWindowConfig.from_buffer_copy(cfg); bad.pyr.levels = 0
    assert capi.keyframe_prepare_plan_raw(C.byref(bad), n.ctypes.data, 2, None, None, None, None) == INVALID


def test_fingerprint_is_bit_equality_of_what_prepare_reads():
    cfg = config(32, 48)
    same = capi.SageWindowConfig.from_buffer_copy(cfg)
    assert capi.keyframe_config_matches(cfg, same)
    # what prepare does not read does not count
    same.CS, same.geo_weight, same.eps, same.use_geo, same.mask_dev = 16, 0.5, 1e-3, 0, 4096
    assert capi.keyframe_config_matches(cfg, same)

    def changed(edit):
        c = capi.SageWindowConfig.from_buffer_copy(cfg)
        edit(c)
        return c

    def ulp(x):
        return float(np.nextafter(np.float32(x), np.float32(1e9)))

    def weight(c): c.photo_weights[1] = ulp(c.photo_weights[1])
    def fx1(c): c.pyr.cam[1].fx = ulp(c.pyr.cam[1].fx)
    def offsets(c): c.pyr.level_offsets[1] += 1
    def fs(c): c.FS = 32
    def levels(c): c.pyr.levels = 1
    for edit in (weight, fx1, offsets, fs, levels):
        assert not capi.keyframe_config_matches(cfg, changed(edit)), edit.__name__
        assert not capi.keyframe_config_matches(changed(edit), cfg), edit.__name__
    assert not capi.keyframe_config_matches(cfg, config(40, 48))                     # another pyramid
    f = capi.lib().sage_keyframe_config_matches
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(None, C.byref(cfg)) == INVALID and f(C.byref(cfg), None) == INVALID


def test_null_and_zero_arguments_return_statuses():
    L = capi.lib()
    cfg = config(32, 48)
    view = capi.SageKeyframeView()
    out = C.c_void_p(0xdead)                              # a refused call leaves NULL, and comes back before the device
    assert capi.keyframe_prepare_batch_raw(None, C.byref(cfg), C.byref(view), 1, C.byref(out)) == INVALID
    assert out.value is None
    assert capi.keyframe_prepare_batch_raw(None, None, None, 0, None) == INVALID
    L.sage_keyframe_prepare.argtypes = [C.c_void_p] * 4
    assert L.sage_keyframe_prepare(None, None, None, None) == INVALID
    L.sage_keyframe_prepare_launches.argtypes = [C.c_void_p]
    assert L.sage_keyframe_prepare_launches(None) == INVALID
    L.sage_keyframe_info.argtypes = [C.c_void_p, C.c_void_p]
    assert L.sage_keyframe_info(None, None) == INVALID
    L.sage_keyframe_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    assert L.sage_keyframe_get(None, 0, None, 0) == INVALID
    L.sage_keyframe_release(None)                          # no-op
    L.sage_window_add_prepared_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    assert L.sage_window_add_prepared_keyframe(None, None, None, None, 0.0) == INVALID
    L.sage_window_build_stats.argtypes = [C.c_void_p, C.c_void_p]
    assert L.sage_window_build_stats(None, None) == INVALID
