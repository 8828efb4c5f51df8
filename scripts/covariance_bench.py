#!/usr/bin/env python3
"""What the marginal covariances cost, one JSON line per window (medians taken in this one process), at K = 16 and K = 64 of the
BASELINE shape 128 x 160 x 16, CS = 32:

  * covariance: ms per sage_window_covariance (the backward recursion over the factor, on the calling thread) next to the ms
    of the sage_window_solve it follows (damping 0, step norm asked for: the stream drained), alternating.
  * sigma kernel: us of depth_sigma_kernel over all K keyframes next to depth_batch_kernel over the same keyframes -- the same
    bytes, 4 (CS + 2) per pixel -- alternating in one process between HIP events (sage_window_depth_sigma_timing), and the
    fraction of 8 TB/s those bytes make.
    Numbers to report; no threshold applies to them.

    python scripts/covariance_bench.py [--steps 40 --warmup 8 --out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def med(x, scale=1e3):
    return round(scale * float(np.median(x)), 4)


def window_row(capi, torch, synth, K, steps, warmup):
    H, W, CS = 128, 160, 32
    w = synth.make_window(K=K, H=H, W=W, FS=16, CS=CS, L=4, seed=0)
    win = capi.Window(w)
    win.linearize()
    t_solve, t_cov = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        win.solve(0.0)
        t1 = time.perf_counter()
        win.covariance()
        t2 = time.perf_counter()
        if i >= warmup:
            t_solve.append(t1 - t0); t_cov.append(t2 - t1)
    win.depth_sigma_timing(warmup)
    sigma_us, depth_us = win.depth_sigma_timing(steps)
    var_us, _ = win.depth_sigma_timing(steps, capi.DEPTH_VARIANCE)
    nbytes = K * H * W * 4 * (CS + 2)
    sig = win.depth_sigma([0])
    torch.cuda.synchronize()
    row = dict(config=f"{H}x{W}x16 CS{CS} K{K}", links=len(win.links), solve_ms=med(t_solve), covariance_ms=med(t_cov),
               depth_sigma_kernel_us=round(sigma_us, 2), depth_variance_kernel_us=round(var_us, 2),
               depth_batch_kernel_us=round(depth_us, 2), bytes=nbytes,
               sigma_fraction_of_8TBs=round(nbytes / (sigma_us * 1e-6) / HBM_BYTES_PER_S, 3),
               depth_batch_fraction_of_8TBs=round(nbytes / (depth_us * 1e-6) / HBM_BYTES_PER_S, 3),
               median_sigma_kf0=round(float(sig.median()), 4))
    win.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_bench.txt"))
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    capi.lib()
    lines = [dict(bench="covariance", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
                  method="medians in one process, ways alternating, warm-up first; kernels by HIP events on the window's stream")]
    for K in (16, 64):
        lines.append(window_row(capi, torch, synth, K, args.steps, args.warmup))
    text = "".join(json.dumps(ln) + "\n" for ln in lines)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
