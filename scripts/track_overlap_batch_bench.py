#!/usr/bin/env python3
"""The overlap statistics of B tracked poses (the loop detector's candidates of one query) timed as one
sage_track_overlap_batch next to the B sage_track_overlap calls it replaces, on the same workspace, in one process,
alternating.

Sizes: the 128 x 160 and 256 x 320 masks of synth.make_overlap_problem (M = 14 528 and 58 052); B = 1, 2, 4, 8, 20, 32; the
poses cycle through synth.OVERLAP_POSES, row b with depth_scale 1 + 0.01 b.  Per (size, B), ms per call as median [min max]
over the timed windows (every window: `calls` calls behind a warm-up of both sides, ended by a device synchronise):
  batch_ms      one sage_track_overlap_batch: three launches, one wait, B + 1 host hulls
  singles_ms    B sage_track_overlap calls: 3 B launches, B waits, 2 B host hulls
  ratio         singles_ms / batch_ms (medians)
  spread        (max - min) / median of either side's windows: what a difference has to exceed to mean anything
  n_candidates  the points that reached the host hull: the input set's (once per batch), then the B warped sets' sum
  launches      what the batch spent (sage_track_overlap_batch_launches) next to the singles' 3 B
The script asserts that every row of the batch is the single call's, byte for byte.  No time here is a pass criterion.
Prints one JSON line per (size, B).

    python scripts/track_overlap_batch_bench.py [--calls 100 --windows 7 --sizes 128x160,256x320 --out FILE]
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

BS = (1, 2, 4, 8, 20, 32)


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
    names = list(synth.OVERLAP_POSES)
    lines = []
    ws = capi.Workspace()
    for H, W in ((int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        prob = synth.make_overlap_problem(H, W, seed=0)
        cam, M = prob["cam"], prob["M"]
        dv = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        dpts, homo, mask = dv(prob["dpts0"]), dv(prob["homo"]), dv(prob["mask"])
        c = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
        eps = float(prob["eps"])
        for B in BS:
            rows = []
            for b in range(B):
                rot, tr = synth.OVERLAP_POSES[names[b % len(names)]]
                rows.append(capi.overlap_pose(synth.so3_exp(np.asarray(rot, np.float64)), tr, 1.0 + 0.01 * b))
            poses = (capi.SageOverlapPose * B)(*rows)
            out_b = (capi.SageOverlapStats * B)()
            out_s = (capi.SageOverlapStats * B)()
            # arguments built once, the calls themselves timed
            batch_args = (ws.h, C.addressof(poses), B, capi.dptr(dpts), capi.dptr(homo), M, C.addressof(c), capi.dptr(mask), eps,
                          C.addressof(out_b))
            single_args = [(ws.h, C.addressof(poses[b].R), C.addressof(poses[b].t), capi.dptr(dpts), float(poses[b].depth_scale),
                            capi.dptr(homo), M, C.addressof(c), capi.dptr(mask), eps, C.addressof(out_s[b])) for b in range(B)]

            def batch():
                rc = capi.track_overlap_batch_raw(*batch_args)
                assert rc == 0, rc

            def singles():
                for args in single_args:
                    rc = capi.track_overlap_raw(*args)
                    assert rc == 0, rc

            batch()
            singles()
            assert bytes(out_b) == bytes(out_s), "batch != singles"
            launches = capi.track_overlap_batch_launches(ws)
            t = alternate_ms(dict(batch_ms=batch, singles_ms=singles), a.calls, a.windows, sync)
            assert bytes(out_b) == bytes(out_s), "batch != singles"
            med = {k: float(np.median(v)) for k, v in t.items()}
            rec = dict(size=f"{H}x{W}", M=M, B=B,
                       batch_ms=[round(med["batch_ms"], 4), round(min(t["batch_ms"]), 4), round(max(t["batch_ms"]), 4)],
                       singles_ms=[round(med["singles_ms"], 4), round(min(t["singles_ms"]), 4), round(max(t["singles_ms"]), 4)],
                       ratio=round(med["singles_ms"] / med["batch_ms"], 3),
                       spread={k: round((max(v) - min(v)) / med[k], 3) for k, v in t.items()},
                       n_candidates=[int(out_b[0].n_candidates[0]), int(sum(o.n_candidates[1] for o in out_b))],
                       launches=dict(batch=launches, singles=3 * B), calls=a.calls, windows=a.windows,
                       device=torch.cuda.get_device_name(0))
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    ws.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
