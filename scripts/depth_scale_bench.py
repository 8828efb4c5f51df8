#!/usr/bin/env python3
"""The mapper's depth-scale correction (sage_depth_scale_ratio; Mapper::CorrectDepthScale) and the device median
(sage_median_f32) timed at the 128 x 160 and 256 x 320 sizes of synth.make_depth_scale_problem, next to the embedder's
alternative today: the literal torch expression of mapper.cpp:248-297 through PyTorch-ROCm on the same device.

Per size:
  depth_scale_ms   one sage_depth_scale_ratio call (depth map + valid locations in, statistics out): the per-point kernel,
                   two histogram passes, the finish, one ticket
  median_ms        one sage_median_f32 call over the keyframe's valid depths (the InitOneFrame normalisation)
  torch_ms         index, matmul, two grid_sample, nonzero, index, median, .item() on cuda tensors
  torch_median_ms  torch.median(dpt_map.reshape(-1)[loc]).item()
Every measurement runs in a child process under a time limit of its own; the first that fails ends the run.  Prints one JSON
line per size.

    python scripts/depth_scale_bench.py [--calls 200 --sizes 128x160,256x320 --out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn, calls, sync):
    for _ in range(5):
        fn()
    sync()
    best = []
    for _ in range(3):                      # median of three batches
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        best.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(best))


def child(H, W, calls):
    import ctypes as C
    import torch
    import torch.nn.functional as F
    from sage_slam_amd import capi, synth
    prob = synth.make_depth_scale_problem(H, W, "small", 0, 1.7)
    cam, M = prob["cam"], prob["M"]
    dv = lambda x, t=np.float32: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()
    dmap, loc, homo = dv(prob["dpt0_map"]), dv(prob["loc1d0"], np.int64), dv(prob["homo"])
    bias1, mask = dv(prob["bias1"]), dv(prob["mask"])
    ws = capi.Workspace()
    sync = torch.cuda.synchronize
    st = capi.depth_scale_ratio(ws, prob["R"], prob["t"], dmap, homo, cam, bias1, mask, prob["eps"], False, loc)
    # --- the engine: arguments built once, the call itself timed
    R = np.ascontiguousarray(prob["R"], np.float32).reshape(9); t = np.ascontiguousarray(prob["t"], np.float32)
    c = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    out = capi.SageDepthScaleStats()
    args = (ws.h, R.ctypes.data, t.ctypes.data, capi.dptr(dmap), capi.dptr(loc), capi.dptr(homo), M, C.addressof(c),
            capi.dptr(bias1), capi.dptr(mask), float(prob["eps"]), 0, None, None, C.addressof(out))
    depth_scale_ms = timed_ms(lambda: capi.depth_scale_ratio_raw(*args), calls, sync)
    med = C.c_float()
    margs = (ws.h, capi.dptr(dmap), capi.dptr(loc), M, 0, C.addressof(med), None, None)
    median_ms = timed_ms(lambda: capi.median_f32_raw(*margs), calls, sync)

    # --- the embedder's alternative: mapper.cpp:248-297
    Rd, td = dv(prob["R"]), dv(prob["t"])
    eps, fx, fy, u0, v0, w, h = (float(v) for v in (prob["eps"], cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h))
    mask4, bias4 = mask.reshape(1, 1, H, W), bias1.reshape(1, 1, H, W)

    def torch_way():
        d0 = dmap.reshape(-1)[loc]
        X = d0.reshape(-1, 1) * torch.matmul(Rd, homo.permute(1, 0)).permute(1, 0) + td.reshape(1, 3)
        pos = X[:, 2] > eps
        Xh = X / X[:, 2:3]
        x2d, y2d = Xh[:, 0:1] * fx + u0, Xh[:, 1:2] * fy + v0
        grid = torch.cat([(x2d + 0.5) * (2.0 / w) - 1.0, (y2d + 0.5) * (2.0 / h) - 1.0], 1).reshape(1, 1, -1, 2)
        d1 = F.grid_sample(bias4, grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(-1)
        vm = F.grid_sample(mask4, grid, mode="nearest", padding_mode="zeros", align_corners=False).reshape(-1) * pos
        ratios = ((X[:, 2] * vm) / d1).reshape(-1)
        return torch.median(ratios[torch.nonzero(vm > 0.5).reshape(-1)]).item()

    torch_ratio = torch_way()
    n_ref = max(calls // 4, 10)
    torch_ms = timed_ms(torch_way, n_ref, sync)
    torch_median = torch.median(dmap.reshape(-1)[loc]).item()
    torch_median_ms = timed_ms(lambda: torch.median(dmap.reshape(-1)[loc]).item(), n_ref, sync)
    capi.median_f32_raw(*margs)
    ws.close()
    return dict(what="depth_scale", size=f"{H}x{W}", M=M, n_selected=int(st.n_selected), depth_scale_ms=depth_scale_ms,
                torch_ms=torch_ms, median_ms=median_ms, torch_median_ms=torch_median_ms, ratio=float(st.ratio),
                torch_ratio=float(torch_ratio), median=float(med.value), torch_median=float(torch_median),
                true_scale=prob["true_scale"], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", default="128x160,256x320")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per measurement (child process)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--child", nargs="*", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(int(args.child[0]), int(args.child[1]), args.calls)))
        return 0
    lines = []
    for h, w in (s.split("x") for s in args.sizes.split(",")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--child", h, w],
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"depth_scale_bench: {h}x{w} ran into its {args.timeout} s limit; stopping", file=sys.stderr)
            return 124
        got = [l[7:] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"depth_scale_bench: {h}x{w} failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}",
                  file=sys.stderr)
            return r.returncode or 1
        print(got[0], flush=True)
        lines.append(got[0])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
