#!/usr/bin/env python3
"""What building a window costs, from views and from prepared keyframes (sage_keyframe_prepare_batch +
sage_window_add_prepared_keyframe), one JSON line per configuration:

  * finalize: wall clock around sage_window_finalize (the device idle before and after) for a window whose keyframes were added
    as views next to the same window added by handle -- K = 16 and K = 64 at 128 x 160 x 16 (CS 32), and BASELINE config 4's
    shape (256 x 320 x 32) at K = 16.  From views is the untouched path: every keyframe relaid, ordered and pre-sampled
    inside the call.  The two ways alternate build by build in this one process; warm-up builds first, then the median.
  * prepare: sage_keyframe_prepare_batch over B = 1, 8, 32, 64 keyframes next to B single calls, per keyframe.
  * sliding: 20 successive 16-keyframe windows, each the previous one moved on by one keyframe (the mapper's loop: a window
    per new keyframe).  From views every window prepares all 16 again; from handles the first prepares 16 in one batch, each
    later one its single new keyframe, and every window borrows.  Total time of create + add + finalize + destroy (+ prepare)
    over the 20 windows; the two ways alternate scenario by scenario.

    python scripts/window_build_bench.py [--builds 12 --warmup 3 --out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Builder:
    """builds windows over the keyframes of one synthetic window through the C calls, so that finalize can be timed alone"""

    def __init__(self, capi, torch, w):
        self.capi, self.torch, self.w, self.L = capi, torch, w, capi.lib()
        self.dks = [capi.DeviceKeyframe(kf, w.H, w.W) for kf in w.keyframes]
        self.mask = capi._dev(w.mask, np.float32)
        cfg = capi.prepare_config(w)
        cfg.mask_dev = self.mask.data_ptr()
        cfg.geo_weight, cfg.geo_loss_param, cfg.eps = w.geo_weight, w.geo_loss_param, w.eps
        cfg.code_prior_weight, cfg.scale_prior_weight, cfg.pose_prior_weight = 1.0e-3, 1.0e4, 1.0e4
        cfg.use_photo, cfg.use_geo = 1, 1
        self.cfg = cfg
        self.vars = [(capi.pack_pose(kf.R, kf.t), np.ascontiguousarray(kf.code, np.float32), float(kf.scale)) for kf in w.keyframes]
        self.add_prepared = self.L.sage_window_add_prepared_keyframe
        self.add_prepared.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]

    def build(self, first, count, handles=None):
        """window over keyframes [first, first + count), by handle where `handles` has one -> (window, finalize seconds)"""
        capi, L = self.capi, self.L
        h = C.c_void_p()
        capi._chk(L.sage_window_create(C.byref(self.cfg), None, C.byref(h)), "sage_window_create")
        for k in range(first, first + count):
            pose, code, scale = self.vars[k]
            if handles is not None and k in handles:
                r = self.add_prepared(h, handles[k].h, pose.ctypes.data, code.ctypes.data, scale)
            else:
                v = self.dks[k].view()
                r = L.sage_window_add_keyframe(h, C.byref(v), capi._fp(pose), capi._fp(code), C.c_float(scale))
            assert r == k - first, r
        for a, b in self.w.links:
            if first <= a < first + count and first <= b < first + count:
                assert L.sage_window_add_link(h, a - first, b - first) >= 0
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi._chk(L.sage_window_finalize(h), "sage_window_finalize")
        self.torch.cuda.synchronize()
        return h, time.perf_counter() - t0

    def destroy(self, h):
        self.L.sage_window_destroy(h)

    def launches(self, h):
        f = self.L.sage_window_build_stats
        f.argtypes = [C.c_void_p, C.c_void_p]
        s = self.capi.SageWindowBuildStats()
        assert f(h, C.byref(s)) == 0
        return int(s.launches)


def med_ms(samples):
    return round(1e3 * float(np.median(samples)), 4)


def finalize_pair(b, ws, K, builds, warmup):
    capi = b.capi
    hs = dict(enumerate(capi.PreparedKeyframe.prepare_batch(ws, b.cfg, b.dks[:K])))
    t = {"views": [], "handles": []}
    n_launch = {}
    for i in range(warmup + builds):
        for way, handles in (("views", None), ("handles", hs)):
            h, sec = b.build(0, K, handles)
            n_launch[way] = b.launches(h)
            b.destroy(h)
            if i >= warmup:
                t[way].append(sec)
    for h in hs.values():
        h.release()
    v, p = med_ms(t["views"]), med_ms(t["handles"])
    return dict(finalize_from_views_ms=v, finalize_from_handles_ms=p, ratio=round(v / p, 3), builds=builds,
                stage_launches_views=n_launch["views"], stage_launches_handles=n_launch["handles"])


def prepare_rows(b, ws, builds, warmup):
    capi, rows = b.capi, []
    for B in (1, 8, 32, 64):
        if B > len(b.dks):
            continue
        tb, ts = [], []
        for i in range(warmup + builds):
            b.torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs = capi.PreparedKeyframe.prepare_batch(ws, b.cfg, b.dks[:B])
            t1 = time.perf_counter()
            singles = [capi.PreparedKeyframe.prepare(ws, b.cfg, dk) for dk in b.dks[:B]]
            t2 = time.perf_counter()
            for h in hs + singles:
                h.release()
            if i >= warmup:
                tb.append((t1 - t0) / B)
                ts.append((t2 - t1) / B)
        rows.append(dict(B=B, batch_ms_per_keyframe=med_ms(tb), single_calls_ms_per_keyframe=med_ms(ts),
                         launches_of_the_batch=capi.keyframe_prepare_plan(b.cfg, [b.dks[0].N] * B)["launches"]))
    return rows


def sliding(b, ws, builds, warmup, windows=20, K=16):
    capi = b.capi
    t = {"views": [], "handles": []}
    for i in range(warmup + builds):
        for way in ("views", "handles"):
            b.torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs = {}
            for s in range(windows):
                if way == "handles":
                    new = [k for k in range(s, s + K) if k not in hs]
                    hs.update(zip(new, capi.PreparedKeyframe.prepare_batch(ws, b.cfg, [b.dks[k] for k in new])))
                    if s > 0:
                        hs.pop(s - 1).release()          # the keyframe that left the window
                h, _ = b.build(s, K, hs if way == "handles" else None)
                b.destroy(h)
            sec = time.perf_counter() - t0
            for h in hs.values():
                h.release()
            if i >= warmup:
                t[way].append(sec)
    v, p = med_ms(t["views"]), med_ms(t["handles"])
    return dict(windows=windows, K=K, total_from_views_ms=v, total_from_handles_ms=p, ratio=round(v / p, 3), runs=builds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=12, help="timed builds per way (>= 10)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    assert args.builds >= 10
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "window_build_bench.py measures on the GPU"
    ws = capi.Workspace()
    lines = [dict(bench="window_build", device=torch.cuda.get_device_name(0), method="median wall clock, ways alternating in one "
                  "process, warm-up builds first", builds=args.builds, warmup=args.warmup)]
    w = synth.make_window(K=64, H=128, W=160, FS=16, CS=32, L=4, seed=0)
    b = Builder(capi, torch, w)
    for K in (16, 64):
        lines.append(dict(config=f"128x160x16 CS32 K{K}", **finalize_pair(b, ws, K, args.builds, args.warmup)))
    lines.append(dict(config="128x160x16 CS32 prepare", rows=prepare_rows(b, ws, args.builds, args.warmup)))
    lines.append(dict(config="128x160x16 CS32 sliding", **sliding(b, ws, args.builds, args.warmup)))
    del b
    w4 = synth.make_window(K=16, H=256, W=320, FS=32, CS=32, L=4, seed=0)
    b4 = Builder(capi, torch, w4)
    lines.append(dict(config="256x320x32 CS32 K16 (config 4)", **finalize_pair(b4, ws, 16, args.builds, args.warmup)))
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
