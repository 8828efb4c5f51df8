#!/usr/bin/env python3
"""The depth-scale corrections of B accepted loop candidates timed as one sage_depth_scale_ratio_batch next to the B
sage_depth_scale_ratio calls it replaces, the same for medians, and sage_loop_accept next to the same steps made of single
calls -- on one workspace, in one process, alternating.

Sizes: the 128 x 160 and 256 x 320 problems of synth.make_depth_scale_problem (M = 14 528 and 58 052), row b with the pose
of synth.OVERLAP_POSES[b mod n] against the keyframe to scale of the "small" pose; B = 1, 4, 9, 20, 32; and one batch of
mixed sizes (M = 1, 2, 255, 256, 257, 2176, 14 528 cut from the first points).  Per line, ms per call as median [min max]
over the timed windows (every window: `calls` calls behind a warm-up of both sides, ended by a device synchronise):
  batch_ms      one batched call: five launches, one wait
  singles_ms    B single calls: 5 B launches, B waits
  ratio         singles_ms / batch_ms (medians)
  spread        (max - min) / median of either side's windows: what a difference has to exceed to mean anything
what = "depth_scale" | "median" (sage_median_f32_batch over the rows' depth maps at their valid locations) | "loop_accept"
(B = 20, all accepted: sage_loop_accept against B sage_depth_scale_ratio calls -- the pose, sort and filter of the singles'
side are not timed, they are microseconds of host arithmetic).
The script asserts that every row of a batch is the single call's, byte for byte.  No time here is a pass criterion.
Prints one JSON line per measurement.

    python scripts/depth_scale_batch_bench.py [--calls 100 --windows 7 --sizes 128x160,256x320 --out FILE]
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

BS = (1, 4, 9, 20, 32)
MIXED = (1, 2, 255, 256, 257, 2176, 14528)


def alternate_ms(fns, calls, windows, sync):
    """fns: name -> callable; timed in turn, window by window, the order swapped every window -> name -> list of ms per call"""
    for fn in fns.values():
        for _ in range(max(calls // 10, 5)):
            fn()
    sync()
    got = {k: [] for k in fns}
    names = list(fns)
    for w in range(windows):
        for k in (names if w % 2 == 0 else names[::-1]):
            fn = fns[k]
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            got[k].append(1e3 * (time.perf_counter() - t0) / calls)
    return got


def record(t, **kw):
    med = {k: float(np.median(v)) for k, v in t.items()}
    rec = dict(kw)
    for k, v in t.items():
        rec[k] = [round(med[k], 4), round(min(v), 4), round(max(v), 4)]
    rec["ratio"] = round(med["singles_ms"] / med["batch_ms"], 3)
    rec["spread"] = {k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="128x160,256x320")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    sync = torch.cuda.synchronize
    device = torch.cuda.get_device_name(0)
    pose_names = list(synth.OVERLAP_POSES)
    dv = lambda x, t=np.float32: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()
    lines = []

    def emit(rec):
        line = json.dumps(dict(rec, calls=a.calls, windows=a.windows, device=device))
        print(line, flush=True)
        lines.append(line)

    ws = capi.Workspace()
    for H, W in ((int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        prob = synth.make_depth_scale_problem(H, W, "small", 0, 1.7)
        cam, M, eps = prob["cam"], prob["M"], float(prob["eps"])
        c = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
        dmap, loc, homo = dv(prob["dpt0_map"]), dv(prob["loc1d0"], np.int64), dv(prob["homo"])
        bias1, mask = dv(prob["bias1"]), dv(prob["mask"])

        def rows_of(Ms):
            rows = []
            for b, m in enumerate(Ms):
                rot, tr = synth.OVERLAP_POSES[pose_names[b % len(pose_names)]]
                rows.append(capi.depth_scale_row(synth.so3_exp(np.asarray(rot, np.float64)), tr, dmap, homo, loc, None, None, m))
            return rows

        def measure(what, Ms, size):
            B = len(Ms)
            rows = (capi.SageDepthScaleRow * B)(*rows_of(Ms))
            out_b, out_s = (capi.SageDepthScaleStats * B)(), (capi.SageDepthScaleStats * B)()
            if what == "depth_scale":
                batch_args = (ws.h, C.addressof(rows), B, C.addressof(c), capi.dptr(bias1), capi.dptr(mask), eps, 1, C.addressof(out_b))
                single_args = [(ws.h, C.addressof(rows[b].R10), C.addressof(rows[b].t10), capi.dptr(dmap), capi.dptr(loc), capi.dptr(homo),
                                Ms[b], C.addressof(c), capi.dptr(bias1), capi.dptr(mask), eps, 1, None, None, C.addressof(out_s[b]))
                               for b in range(B)]
                call_b, call_s = capi.depth_scale_ratio_batch_raw, capi.depth_scale_ratio_raw
                results = lambda: (bytes(out_b), bytes(out_s))
            else:
                vp = (C.c_void_p * B)(*([capi.dptr(dmap).value] * B))
                lp = (C.c_void_p * B)(*([capi.dptr(loc).value] * B))
                n = (C.c_int32 * B)(*Ms)
                med_b, med_s = (C.c_float * B)(), (C.c_float * B)()
                batch_args = (ws.h, C.addressof(vp), C.addressof(lp), C.addressof(n), B, 0, C.addressof(med_b), None, None)
                single_args = [(ws.h, capi.dptr(dmap), capi.dptr(loc), Ms[b], 0, C.addressof(med_s) + 4 * b, None, None) for b in range(B)]
                call_b, call_s = capi.median_f32_batch_raw, capi.median_f32_raw
                results = lambda: (bytes(med_b), bytes(med_s))

            def batch():
                rc = call_b(*batch_args)
                assert rc == 0, rc

            def singles():
                for args in single_args:
                    rc = call_s(*args)
                    assert rc == 0, rc

            batch()
            singles()
            assert len(set(results())) == 1, "batch != singles"
            launches = capi.depth_scale_ratio_batch_launches(ws)
            t = alternate_ms(dict(batch_ms=batch, singles_ms=singles), a.calls, a.windows, sync)
            assert len(set(results())) == 1, "batch != singles"
            emit(record(t, what=what, size=size, B=B, M=Ms[0] if len(set(Ms)) == 1 else list(Ms),
                        launches=dict(batch=launches, singles=5 * B)))

        for B in BS:
            measure("depth_scale", [M] * B, f"{H}x{W}")
        for B in BS:
            measure("median", [M] * B, f"{H}x{W}")
        if (H, W) == (128, 160):
            measure("depth_scale", [m for m in MIXED if m <= M], f"{H}x{W} mixed")

        # sage_loop_accept at B = 20, every candidate accepted, against the 20 single corrections it replaces
        B = 20
        cands = (capi.SageLoopCandidate * B)()
        scands = (capi.SageLoopScaleCandidate * B)()
        pre = (capi.SageLoopPrecheckResult * B)()
        ver = (capi.SageLoopVerifyResult * B)()
        rows = rows_of([M] * B)
        for b in range(B):
            cands[b].dpt_map_dev = capi.dptr(dmap).value
            scands[b] = capi.SageLoopScaleCandidate(10 * b, capi.dptr(loc).value, capi.dptr(homo).value, M, 1.0, 1.0)
            pre[b].desc_match_inlier_ratio = 0.5 + 0.01 * b
            v = ver[b]
            v.tracked, v.status, v.area_ratio, v.inlier_ratio, v.area_inlier_ratio = 1, 0, 0.9, 0.9, 0.81
            R, t = np.array(rows[b].R10[:], np.float32).reshape(3, 3), np.array(rows[b].t10[:], np.float32)
            v.pose12[:] = [float(x) for x in np.concatenate([R.T.reshape(9), -(R.T @ t)])]
        cfg = capi.SageLoopAcceptConfig(0.5, 0.5, 0.3, 0.2, 5, eps)
        q = capi.SageLoopScaleQuery(capi.dptr(bias1).value, capi.dptr(mask).value, c)
        infos = (capi.SageLoopInfo * B)()
        kept = (C.c_int32 * B)()
        n_kept = C.c_int32()
        accept_args = (ws.h, C.addressof(cfg), C.addressof(q), C.addressof(cands), C.addressof(scands), C.addressof(pre), C.addressof(ver),
                       B, C.addressof(infos), C.addressof(kept), C.addressof(n_kept))
        out_s = (capi.SageDepthScaleStats * B)()

        def accept():
            rc = capi.loop_accept_raw(*accept_args)
            assert rc == 0, rc

        accept()
        assert n_kept.value == B and all(infos[b].accepted for b in range(B))
        single_args = [(ws.h, C.addressof(infos[b].R_cur_ref), C.addressof(infos[b].t_cur_ref), capi.dptr(dmap), capi.dptr(loc),
                        capi.dptr(homo), M, C.addressof(c), capi.dptr(bias1), capi.dptr(mask), eps, 1, None, None, C.addressof(out_s[b]))
                       for b in range(B)]

        def singles():
            for args in single_args:
                rc = capi.depth_scale_ratio_raw(*args)
                assert rc == 0, rc

        singles()
        assert all(bytes(infos[b].scale) == bytes(out_s[b]) for b in range(B)), "loop_accept != singles"
        t = alternate_ms(dict(batch_ms=accept, singles_ms=singles), a.calls, a.windows, sync)
        emit(record(t, what="loop_accept", size=f"{H}x{W}", B=B, M=M,
                    launches=dict(batch=capi.depth_scale_ratio_batch_launches(ws), singles=5 * B)))
    ws.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
