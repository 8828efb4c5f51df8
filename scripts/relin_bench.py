#!/usr/bin/env python3
"""What a linearizing prepass costs when only a few keyframes have moved (sage_window_set_relinearization), measured on the
headline window (K = 64 at 128 x 160, dense factors, CS 32) in one process:

  * SAGE_RELIN_ALL: every prepass evaluates the 372 + 372 dense edges, every depth map, and copies every per-edge system;
  * SAGE_RELIN_STALE with the newest 1, 4, 16 and all 64 keyframes changed (pose, code and scale of each, fresh bits every
    time) between two prepasses: the stale edges, the depth maps they read, their rows only.

ms per sage_window_prepass(jacobians = 1) is the median host time of the call, which ends behind a wait on the device and the
copies to the host cache; the SageEvalCounts of the last call of each series are printed next to it.  The expectation -- not a
bar -- is a fixed part (variable upload, terms, assembly, the copy's latency) plus a part roughly linear in the stale edges.

    python scripts/relin_bench.py [--keyframes 64 --height 128 --width 160 --reps 30 --out profiles/relin_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_values(w):
    poses = np.stack([np.concatenate([np.asarray(k.R, np.float32).reshape(-1), np.asarray(k.t, np.float32).reshape(-1)])
                      for k in w.keyframes])
    codes = np.stack([np.asarray(k.code, np.float32).reshape(-1) for k in w.keyframes])
    scales = np.array([k.scale for k in w.keyframes], np.float32)
    return poses, codes, scales


def series(win, vals, n_changed, reps, warmup=5):
    """`reps` timed prepasses, the newest n_changed keyframes changed before each -> (median ms, min ms, last counts)"""
    poses, codes, scales = (a.copy() for a in vals)
    K = poses.shape[0]
    ts = []
    for i in range(reps + warmup):
        sign = np.float32(1.0 if i % 2 == 0 else -1.0)                  # back and forth: the values stay where they are
        poses[K - n_changed:, 9:] += sign * np.float32(1e-4)
        codes[K - n_changed:] += sign * np.float32(1e-4)
        scales[K - n_changed:] *= np.float32(1.0) + sign * np.float32(1e-4)
        t0 = time.perf_counter()
        recomputed = win.prepass(poses, codes, scales, jacobians=True)
        dt = time.perf_counter() - t0
        assert recomputed
        if i >= warmup:
            ts.append(dt)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), win.last_evaluation()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the text report here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "relin_bench.py measures on the GPU"
    K = args.keyframes
    w = synth.make_window(K=K, H=args.height, W=args.width, FS=16, CS=32, L=4, seed=0)
    win = capi.Window(w)
    vals = window_values(w)
    lines = [f"relin_bench: device {torch.cuda.get_device_name(0)}; K {K}, {args.height} x {args.width}, CS 32, {len(w.links)} dense "
             f"links; ms per sage_window_prepass(jacobians = 1), median (min) of {args.reps}"]
    out = {}

    def row(title, key, n_changed):
        med, lo, n = series(win, vals, n_changed, args.reps)
        out[key] = dict(ms=med, ms_min=lo, **n)
        lines.append(f"  {title:<44s} {med:8.3f} ms ({lo:7.3f})   edges {n['photo_edges']:3d} + {n['geo_edges']:3d}, items "
                     f"{n['photo_items']:5d} + {n['geo_items']:5d}, depth maps {n['depth_maps']:2d}, gradients {n['depth_grads']:2d}, "
                     f"rows to the host {n['host_entries_pulled']:3d}")

    row("SAGE_RELIN_ALL, 1 keyframe changed", "all_1", 1)
    row(f"SAGE_RELIN_ALL, all {K} changed", f"all_{K}", K)
    win.set_relinearization(capi.SAGE_RELIN_STALE)
    for n_changed in sorted({1, 4, 16, K} & set(range(1, K + 1))):
        row(f"SAGE_RELIN_STALE, newest {n_changed} changed", f"stale_{n_changed}", n_changed)
    win.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
