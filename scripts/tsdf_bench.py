#!/usr/bin/env python3
"""What TSDF fusion costs, one JSON line per row (medians taken in this one process, the forms alternating inside every
repetition, warm-up first; times between HIP events on the volume's stream, the event pair's own floor stated):

  * volume rows: sage_tsdf_integrate_batch against n calls of sage_tsdf_integrate on volumes of 256^3 and 400^3 voxels (the
    script's default budget of 64 M) with color, n = 16 and 64 views of 128 x 160 (synth.make_tsdf_scene): the batch with and
    without the cull and in the three brick shapes (x 1, 2, 4 voxels per thread).  Next to each time the bytes model --
    n * 24 B * V for the singles, 24 B * V once for the batch, plus the images (12 B per pixel and view) -- the fraction of
    8 TB/s that model makes of the time, the share of brick-view pairs kept, and the per-voxel operation rate (about 40
    fp32 operations per voxel and kept view; 256-voxel-line granularity makes the count an upper bound).
  * window row: sage_window_fuse_tsdf of the 16-keyframe 128 x 160 window (CS 32) in both std modes into a volume planned from
    its own frusta at the script's budget, host clock around a drained stream, next to the LM step of the same window from
    profiles/marginal_prior_bench.txt.
Numbers to report; no threshold applies to them.

    python scripts/tsdf_bench.py [--steps 10 --warmup 2 --out FILE --small]
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
OPS_PER_VOXEL_VIEW = 40


def med(x):
    return float(np.median(x))


def volume_rows(capi, torch, synth, ws, side, n, steps, warmup):
    H, W = 128, 160
    scene = synth.make_tsdf_scene(11, (side, side, side), (H, W), n, voxel_size=0.04 * 24 / side, trunc_voxels=10.0)
    plan = capi.tsdf_plan_exact(scene["dims"], scene["origin"], scene["voxel_size"], scene["trunc_margin"], True)
    vol = capi.TsdfVolume(ws, plan)
    views = []
    for v in scene["views"]:
        t = {k: torch.from_numpy(np.ascontiguousarray(v[k])).cuda() for k in ("depth", "std", "color")}
        views.append(capi.tsdf_view(t["depth"], v["pose12"], scene["cam"], std=t["std"], color=t["color"]))
    forms = [("singles", None), ("batch", 0), ("batch_no_cull", capi.TSDF_NO_CULL), ("batch_x1", capi.TSDF_BRICK_X1),
             ("batch_x2", capi.TSDF_BRICK_X2), ("batch_x4", capi.TSDF_BRICK_X4)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in forms}
    floor, kept = [], {}
    for i in range(warmup + steps):
        a.record(); b.record(); b.synchronize()
        if i >= warmup:
            floor.append(a.elapsed_time(b))
        for name, fl in forms:
            a.record()
            if fl is None:
                for v in views:
                    vol.integrate(v)
            else:
                vol.integrate_batch(views, flags=fl)
            b.record(); b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
            if fl is not None and name not in kept:
                st = vol.last_stats()
                kept[name] = (int(st.pairs_kept), int(st.pairs), list(st.brick))
    V = int(plan.voxels)
    image_bytes = n * H * W * 12
    rows = []
    for name, fl in forms:
        ms = med(times[name])
        model = (n if fl is None else 1) * 24 * V + image_bytes
        row = dict(volume=f"{side}^3", views=n, form=name, ms=round(ms, 4), bytes_model=model,
                   fraction_of_8TBs=round(model / (ms * 1e-3) / HBM_BYTES_PER_S, 4))
        if fl is not None:
            k, p, brick = kept[name]
            row.update(brick=brick, pairs=p, pairs_kept=k, share_kept=round(k / p, 4),
                       gops_per_s=round(OPS_PER_VOXEL_VIEW * k * brick[0] * brick[1] * brick[2] / (ms * 1e-3) / 1e9, 1))
        else:
            row.update(gops_per_s=round(OPS_PER_VOXEL_VIEW * n * V / (ms * 1e-3) / 1e9, 1))
        rows.append(row)
    rows.append(dict(volume=f"{side}^3", views=n, event_pair_floor_ms=round(med(floor), 4),
                     batch_over_singles=round(med(times["batch"]) / med(times["singles"]), 4)))
    vol.close()
    return rows


def lm_step_ms():
    try:
        with open(os.path.join(ROOT, "profiles", "marginal_prior_bench.txt")) as f:
            for line in f:
                row = json.loads(line)
                if row.get("m") == 3 and "lm_step_without_ms" in row:
                    return row["lm_step_without_ms"]
    except (OSError, ValueError):
        pass
    return None


def window_row(capi, torch, synth, ws, steps, warmup, small):
    K, H, W, CS = 16, (32 if small else 128), (40 if small else 160), 32
    w = synth.make_window(K=K, H=H, W=W, FS=16, CS=CS, L=(2 if small else 4), seed=0)
    win = capi.Window(w)
    win.linearize(); win.solve(0.0); win.covariance()
    kfs = list(range(K))
    lo, hi = capi.window_depth_range(win, kfs)
    bounds = np.zeros(6)
    for k in kfs:
        bounds = capi.tsdf_frustum_bounds(w.cams[0], win.get_keyframe(k)[0], hi, bounds)
    plan = capi.tsdf_plan(bounds, 0.1, 1.0e5 if small else 64.0e6, 10.0)
    vol = capi.TsdfVolume(ws, plan)
    times = {capi.TSDF_STD_ONE: [], capi.TSDF_STD_SIGMA: []}
    for i in range(warmup + steps):
        for mode in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.window_fuse_tsdf(win, vol, kfs, mode, 1.0e-3 if mode else 0.0, 1.0, 1.0e-4)
            torch.cuda.synchronize()
            if i >= warmup:
                times[mode].append(time.perf_counter() - t0)
    st = vol.last_stats()
    row = dict(config=f"{H}x{W}x16 CS{CS} K{K}", volume=list(plan.dim), voxels=int(plan.voxels), voxel_size=round(plan.voxel_size, 5),
               depth_range=[round(lo, 4), round(hi, 4)], fuse_std_one_ms=round(1e3 * med(times[capi.TSDF_STD_ONE]), 4),
               fuse_std_sigma_ms=round(1e3 * med(times[capi.TSDF_STD_SIGMA]), 4), share_kept=round(st.pairs_kept / st.pairs, 4),
               lm_step_ms_from_marginal_prior_bench=lm_step_ms())
    win.close(); vol.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from sage_slam_amd import capi, synth
    capi.lib()
    ws = capi.Workspace()
    lines = [dict(bench="tsdf", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, small=args.small,
                  method="medians in one process, forms alternating inside every repetition, warm-up first; HIP events on the "
                         "volume's stream (their own floor per row group); the window row by host clock around a drained stream")]
    for side in ((48,) if args.small else (256, 400)):
        for n in ((3,) if args.small else (16, 64)):
            lines += volume_rows(capi, torch, synth, ws, side, n, args.steps, args.warmup)
    lines.append(window_row(capi, torch, synth, ws, args.steps, args.warmup, args.small))
    ws.close()
    text = "".join(json.dumps(ln) + "\n" for ln in lines)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
