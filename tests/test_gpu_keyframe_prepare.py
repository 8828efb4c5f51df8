"""Prepared keyframes on the device: a window built from handles (``sage_keyframe_prepare`` / ``_batch``, then
``sage_window_add_prepared_keyframe``) computes BIT FOR BIT what its twin built from views computes -- every comparison is on
``tobytes()``, no tolerance: the handle holds the planes, the ordered samples and the pre-sampled source features that stages
3-5 of ``sage_window_finalize`` would have made, and nothing downstream of the edge tables knows who owns them.  K = 4
keyframes, ``back_links=3``, the smallest images at which each ordering rule of ``finalize_samples`` is taken."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from sage_slam_amd import synth

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4
ALIGNED = dict(H=32, W=48, L=2, border=2, erode=6)       # samples rows 8..23 x cols 8..39: whole 8 x 8 tiles
RAGGED = dict(H=38, W=62, L=2, border=2, erode=6)        # rows 8..29 x cols 8..53: 18 tiles, 1012 samples
NON_DYADIC = dict(H=50, W=62, L=3, allow_odd=True, border=2, erode=3)   # tests/test_gpu_parity.py's
CASES = {
    "aligned": dict(args=ALIGNED, info=dict(N=512, slots=512, ordered=1, padded=0)),
    "ragged": dict(args=RAGGED, info=dict(N=1012, slots=64 * 18, ordered=1, padded=1)),
    "sparse": dict(args=dict(ALIGNED, n_samples=200), info=dict(N=200, slots=200, ordered=1, padded=0)),
    "duplicate": dict(args=ALIGNED, info=dict(N=512, slots=512, ordered=0, padded=0)),
    "non_dyadic": dict(args=NON_DYADIC, info=dict(N=(50 - 10) * (62 - 10))),
    "fs32": dict(args=dict(ALIGNED, FS=32), info=dict(N=512, slots=512, ordered=1, padded=0)),
}


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available()
    from sage_slam_amd import capi as c
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


@functools.lru_cache(maxsize=None)
def case_window(name, CS, K=4, seed=7):
    a = dict(CASES[name]["args"])
    a.setdefault("FS", 16)
    w = synth.make_window(K=K, CS=CS, back_links=3, seed=seed, **a)
    if name == "duplicate":
        for kf in w.keyframes:
            kf.loc1d[1] = kf.loc1d[0]
            kf.homo[1] = kf.homo[0]
    return w


def handles_of(capi, ws, w, ks=None):
    """{k: handle} for the keyframes `ks` of w (all), prepared in one batch"""
    ks = list(range(len(w.keyframes))) if ks is None else list(ks)
    dks = [capi.DeviceKeyframe(w.keyframes[k], w.H, w.W) for k in ks]
    return dict(zip(ks, capi.PreparedKeyframe.prepare_batch(ws, capi.prepare_config(w), dks)))


def edge_bytes(win):
    out = []
    for e in range(2 * len(win.win.links)):
        for t in (0, 1):
            r = win.get_edge(t, e)
            out.append(r["AtA"].tobytes() + r["Atb"].tobytes() + np.float32([r["error"], r["num_inliers"]]).tobytes())
    return out


def linearized(win):
    win.linearize()
    return dict(packed=win.packed_host().tobytes(), edges=edge_bytes(win))


def observed(capi, win):
    """everything test 1 compares, as bytes"""
    out = linearized(win)
    assert len(out["packed"]) == 8 * win.packed_count
    win.error(1)
    out["error"] = win.error_tensor().cpu().numpy().tobytes()
    st, cfg = capi.SageLmState(), capi.lm_config_default()
    for _ in range(2):
        win.lm_step(st, cfg)
    out["lm"] = (st.error, st.candidate_error, st.accepted)
    out["keyframes"] = [b"".join([p.tobytes(), c.tobytes(), np.float32(s).tobytes()])
                        for p, c, s in (win.get_keyframe(k) for k in range(win.K))]
    out["delta"] = win.delta().tobytes()
    out["counts"] = (win.residuals_per_linearize, win.bytes_per_linearize)
    return out


def stats(win):
    s = win.build_stats()
    return {n: int(getattr(s, n)) for n, _ in s._fields_}


# ------------------------------------------------------------------------------------------------ 1, 2: whole and mixed windows
@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_window_from_handles_is_byte_equal_to_window_from_views(capi, ws, name, CS):
    w = case_window(name, CS)
    hs = handles_of(capi, ws, w)
    for h in hs.values():
        i = h.info()
        for field, want in CASES[name]["info"].items():
            assert getattr(i, field) == want, (name, field, getattr(i, field))
        assert i.refs == 1
    views, handles, mixed = capi.Window(w), capi.Window(w, prepared=hs), capi.Window(w, prepared={0: hs[0], 2: hs[2]})
    assert [h.info().refs for h in hs.values()] == [3, 2, 3, 2]
    sv, sh, sm = stats(views), stats(handles), stats(mixed)
    assert (sv["prepared"], sv["repacked"], sv["ordered"], sv["presampled"]) == (0, 4, 4, 4)
    assert (sh["prepared"], sh["repacked"], sh["ordered"], sh["presampled"], sh["launches"]) == (4, 0, 0, 0, 0)
    assert (sm["keyframes"], sm["prepared"], sm["repacked"], sm["ordered"], sm["presampled"]) == (4, 2, 2, 2, 2)
    assert sv["launches"] > sm["launches"] > 0
    want = observed(capi, views)
    assert observed(capi, handles) == want
    assert observed(capi, mixed) == want
    for win in (views, handles, mixed):
        win.close()
    assert [h.info().refs for h in hs.values()] == [1, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ 3: sharing and sliding
def sub_window(w, first, count):
    """keyframes [first, first + count) of w with the links among them, renumbered"""
    links = [(a - first, b - first) for a, b in w.links if first <= a < first + count and first <= b < first + count]
    return dataclasses.replace(w, keyframes=w.keyframes[first:first + count], links=links)


def test_two_live_windows_share_handles_and_keep_them_alive(capi, ws):
    w5 = case_window("aligned", 32, K=5)
    hs = handles_of(capi, ws, w5)
    wa, wb = sub_window(w5, 0, 4), sub_window(w5, 1, 4)
    A = capi.Window(wa, prepared={k: hs[k] for k in range(4)})
    B = capi.Window(wb, prepared={k: hs[k + 1] for k in range(4)})
    assert [hs[k].info().refs for k in range(5)] == [2, 3, 3, 3, 2]
    raw = [hs[k].h.value for k in range(5)]
    for h in hs.values():
        h.release()                                       # the callers' references, before any window call
    assert [capi.keyframe_info_raw(C.c_void_p(r)).refs for r in raw] == [1, 2, 2, 2, 1]
    for win, sub in ((A, wa), (B, wb)):
        twin = capi.Window(sub)
        assert stats(win)["launches"] == 0
        assert linearized(win) == linearized(twin)
        twin.close()
    A.close()
    assert [capi.keyframe_info_raw(C.c_void_p(r)).refs for r in raw[1:]] == [1, 1, 1, 1]   # (h0 went with window A)
    B.close()                                             # ... and the rest with window B: nothing is left to query


# ------------------------------------------------------------------------------------------------ 4: batch = single, contents
def tile_walk_key(loc, W):
    y, x = loc // W, loc % W
    return ((y // 8) * ((W + 7) // 8) + x // 8) * 64 + (y % 8) * 8 + x % 8


def relay_numpy(capi, cfg, kf):
    """SAGE_PREP_PACKED restated: (fx_l or fy_l or 1) * sqrt(w_l), then times the texel, in fp32"""
    L, P, FS = cfg.pyr.levels, cfg.pyr.P, cfg.FS
    level = np.zeros(P, np.int64)
    for l in range(1, L):
        level[cfg.pyr.level_offsets[l]:] = l
    sw = np.sqrt(np.float32([cfg.photo_weights[l] for l in range(L)]))
    out = np.zeros((3, FS // 4, P, 4), np.float32)
    srcs = (kf.feat_pyr.reshape(FS, P), kf.grad_pyr.reshape(2, FS, P)[0], kf.grad_pyr.reshape(2, FS, P)[1])
    for a, src in enumerate(srcs):
        f = np.float32([1.0 if a == 0 else (cfg.pyr.cam[l].fx if a == 1 else cfg.pyr.cam[l].fy) for l in range(L)])
        sc = (f * sw).astype(np.float32)[level]                                     # [P]
        out[a] = (sc[None, :] * src.astype(np.float32)).reshape(FS // 4, 4, P).transpose(0, 2, 1)
    return out


def all_arrays(capi, h):
    i = h.info()
    return dict(info=(i.N, i.slots, i.ordered, i.padded, i.device_bytes),
                **{str(what): h.get(what).tobytes() for what in (capi.SAGE_PREP_PACKED, capi.SAGE_PREP_LOC, capi.SAGE_PREP_HOMO,
                                                                  capi.SAGE_PREP_F0S)})


def test_batch_is_byte_equal_to_single_and_holds_the_tile_walk(capi, ws):
    a, other = case_window("aligned", 32), case_window("aligned", 32, seed=8)
    one = synth.make_window(K=1, CS=32, back_links=3, seed=7, FS=16, **dict(ALIGNED, n_samples=1))
    kfs = [a.keyframes[0], case_window("sparse", 32).keyframes[0], case_window("duplicate", 32).keyframes[1],
           other.keyframes[2], one.keyframes[0]]
    cfg = capi.prepare_config(a)
    plan = capi.keyframe_prepare_plan(cfg, [kf.loc1d.size for kf in kfs])
    assert (plan["launches"], plan["waits"]) == (6, 2)
    dks = [capi.DeviceKeyframe(kf, a.H, a.W) for kf in kfs]
    batch = capi.PreparedKeyframe.prepare_batch(ws, cfg, dks)
    n_batch = capi.keyframe_prepare_launches(ws)
    singles = []
    for dk in dks:
        singles.append(capi.PreparedKeyframe.prepare(ws, cfg, dk))
        assert capi.keyframe_prepare_launches(ws) == n_batch == plan["launches"]
    for b, (hb, hs) in enumerate(zip(batch, singles)):
        assert all_arrays(capi, hb) == all_arrays(capi, hs), b
        assert hb.info().device_bytes == plan["device_bytes"][b]
    assert [(h.info().N, h.info().slots, h.info().ordered, h.info().padded) for h in batch] == \
        [(512, 512, 1, 0), (200, 200, 1, 0), (512, 512, 0, 0), (512, 512, 1, 0), (1, 1, 1, 0)]
    for b in (0, 1, 3, 4):                                # ordered: the sorted 8 x 8 tile walk of the input, rays alongside
        order = np.argsort(tile_walk_key(kfs[b].loc1d, a.W), kind="stable")
        assert np.array_equal(batch[b].get(capi.SAGE_PREP_LOC), kfs[b].loc1d[order])
        assert batch[b].get(capi.SAGE_PREP_HOMO).tobytes() == kfs[b].homo[order].tobytes()
    assert np.array_equal(batch[2].get(capi.SAGE_PREP_LOC), kfs[2].loc1d)          # a pixel sampled twice: the caller's order
    for b in (0, 3):
        assert batch[b].get(capi.SAGE_PREP_PACKED).tobytes() == relay_numpy(capi, cfg, kfs[b]).tobytes()
    # two ragged keyframes: the tile-padded order, one launch and one wait more
    r = case_window("ragged", 32)
    rcfg = capi.prepare_config(r)
    rdks = [capi.DeviceKeyframe(r.keyframes[k], r.H, r.W) for k in (0, 1)]
    rb = capi.PreparedKeyframe.prepare_batch(ws, rcfg, rdks)
    assert capi.keyframe_prepare_launches(ws) == plan["launches"] + 1
    for k, (hb, dk) in enumerate(zip(rb, rdks)):
        hs = capi.PreparedKeyframe.prepare(ws, rcfg, dk)
        assert capi.keyframe_prepare_launches(ws) == plan["launches"] + 1
        assert all_arrays(capi, hb) == all_arrays(capi, hs)
        loc, homo = hb.get(capi.SAGE_PREP_LOC), hb.get(capi.SAGE_PREP_HOMO)
        assert loc.size == 1152 and hb.info().padded == 1
        hole = loc < 0
        assert np.all(loc[hole] == -1) and np.all(homo[hole] == np.float32([0, 0, 1]))
        assert np.array_equal(np.sort(loc[~hole]), np.sort(r.keyframes[k].loc1d))          # every sampled pixel exactly once
        slot = np.arange(loc.size)[~hole]
        key = tile_walk_key(loc[~hole], r.W)
        assert np.array_equal(slot % 64, key % 64)                                          # a wave is a tile: slot = place in tile
        assert np.array_equal(slot // 64, np.unique(key // 64, return_inverse=True)[1])     # ... of the s-th sampled tile
        assert hb.get(capi.SAGE_PREP_PACKED).tobytes() == relay_numpy(capi, rcfg, r.keyframes[k]).tobytes()


# ------------------------------------------------------------------------------------------------ 5: statuses
def raw_prepare(capi, ws, cfg, dks, B=None):
    views = (capi.SageKeyframeView * max(1, len(dks)))(*[dk.view() for dk in dks])
    out = (C.c_void_p * max(1, len(dks), B or 0))()
    rc = capi.keyframe_prepare_batch_raw(ws.h, C.byref(cfg), views, len(dks) if B is None else B, out)
    return rc, list(out)


def test_statuses(capi, ws):
    import torch
    w = case_window("aligned", 32)
    cfg = capi.prepare_config(w)
    dk = capi.DeviceKeyframe(w.keyframes[0], w.H, w.W)
    good = capi.PreparedKeyframe.prepare(ws, cfg, dk)
    # handles a window of `w` must refuse: other level weights, another FS, another pyramid
    cfg_w = capi.prepare_config(w)
    cfg_w.photo_weights[1] = float(np.nextafter(np.float32(cfg_w.photo_weights[1]), np.float32(100)))
    w_fs, w_pyr = case_window("fs32", 32), synth.make_window(K=1, H=40, W=48, L=2, CS=32, seed=7)
    bad = [capi.PreparedKeyframe.prepare(ws, cfg_w, dk),
           capi.PreparedKeyframe.prepare(ws, capi.prepare_config(w_fs), capi.DeviceKeyframe(w_fs.keyframes[0], w.H, w.W)),
           capi.PreparedKeyframe.prepare(ws, capi.prepare_config(w_pyr), capi.DeviceKeyframe(w_pyr.keyframes[0], 40, 48))]
    twin = capi.Window(w)
    L = capi.lib()
    blank = object.__new__(capi.Window)                   # an unfinalized window of the twin's configuration
    blank.h, blank.win = C.c_void_p(), w
    assert L.sage_window_create(C.byref(twin.cfg), None, C.byref(blank.h)) == 0
    kf0 = w.keyframes[0]
    pose = capi.pack_pose(kf0.R, kf0.t)
    for h in bad:
        assert blank.add_prepared_keyframe(h, pose, kf0.code, kf0.scale) == INVALID
        assert h.info().refs == 1
    assert blank.add_prepared_keyframe(None, pose, kf0.code, kf0.scale) == INVALID
    assert blank.add_prepared_keyframe(good, pose, kf0.code, kf0.scale) == 0         # ... and is still usable: handle 0, views 1..3
    for k in (1, 2, 3):
        kf, v = w.keyframes[k], twin.kfs[k].view()
        p, c = capi.pack_pose(kf.R, kf.t), np.ascontiguousarray(kf.code, np.float32)
        assert L.sage_window_add_keyframe(blank.h, C.byref(v), capi._fp(p), capi._fp(c), C.c_float(kf.scale)) == k
    for l, (a, b) in enumerate(w.links):
        assert L.sage_window_add_link(blank.h, a, b) == l
    assert L.sage_window_finalize(blank.h) == 0
    blank.K, blank.packed_count = 4, L.sage_window_packed_count(blank.h)
    assert linearized(blank) == linearized(twin)
    assert blank.add_prepared_keyframe(good, pose, kf0.code, kf0.scale) == STATE     # after finalize
    assert good.info().refs == 2
    blank.close(); twin.close()
    # prepare: a location == H * W, a negative level weight, B = 0 and B = 65 -- nothing launched after the refusal
    plan = capi.keyframe_prepare_plan(cfg, [512])
    out_of_image = capi.DeviceKeyframe(w.keyframes[1], w.H, w.W)
    out_of_image.loc1d = out_of_image.loc1d.clone()
    out_of_image.loc1d[5] = w.H * w.W
    torch.cuda.synchronize()
    rc, out = raw_prepare(capi, ws, cfg, [out_of_image])
    assert rc == INVALID and out[0] is None
    assert capi.keyframe_prepare_launches(ws) == plan["launches"] - 1               # the relay and the sort; no pre-sampling
    rc, out = raw_prepare(capi, ws, cfg, [dk, out_of_image, dk])                     # a batch that fails leaves no handle
    assert rc == INVALID and out == [None, None, None]
    neg = capi.prepare_config(w)
    neg.photo_weights[1] = -1.0
    for c_, dks, B in ((neg, [dk], None), (cfg, [dk], 0), (cfg, [dk], 65)):
        rc, out = raw_prepare(capi, ws, c_, dks, B)
        assert rc == INVALID and out[0] is None and capi.keyframe_prepare_launches(ws) == 0


# ------------------------------------------------------------------------------------------------ 6: features on a handle window
def test_stale_relinearization_dogleg_and_factor_cache_on_a_handle_window(capi, ws):
    w = case_window("aligned", 32)
    hs = handles_of(capi, ws, w)
    seen = []
    for win in (capi.Window(w, prepared=hs), capi.Window(w)):
        win.set_relinearization(capi.SAGE_RELIN_STALE)
        out = [linearized(win)]
        pose, code, scale = win.get_keyframe(2)
        win.set_keyframe(2, pose, code, np.float32(scale) * np.float32(1.01))
        win.linearize()
        out.append(win.last_evaluation())
        assert 0 < out[-1]["photo_edges"] < 2 * len(w.links)                       # (stale edges only: the mode is on)
        st = win.dogleg_step(capi.SageDoglegState(), capi.dogleg_config_default())
        out.append(bytes(st))
        out.append([np.concatenate([p, c, [s]]).tobytes() for p, c, s in (win.get_keyframe(k) for k in range(4))])
        poses = np.stack([capi.pack_pose(k.R, k.t) for k in w.keyframes])
        codes = np.stack([np.asarray(k.code, np.float32) for k in w.keyframes])
        assert win.prepass(poses, codes, np.float32([k.scale for k in w.keyframes]), jacobians=True)
        blocks, gs, f, dims = win.factor(0, 0)
        out.append((b"".join(blocks[k].tobytes() for k in blocks), b"".join(np.asarray(g).tobytes() for g in gs), f, dims))
        seen.append(out)
        win.close()
    assert seen[0] == seen[1]
