#!/usr/bin/env python3
"""The loop-closure pose-scale graph (DeepFactors::LoopClosurePoseScaleMGEstimate) as a window of the batched engine, measured:
K = 512 keyframes at 64 x 80 on a circle, the links of the synthetic window (three back links per keyframe) plus the loop
closures of BASELINE config 5 as KEYPOINT links -- no dense edge at all --, one loop-MG term of 128 points per direction
(fixed depths, D = 14), all codes and keyframe 0 held.

Prints the ms per LM step (median of the steady iterations of sage_window_lm_run_timed) and its phase split on the stream's
timeline (sage_window_get_phase_time: linearize = the one keypoint launch + assembly, solve = scatter + host factorisation +
retract, error pass), the batched kernel's own time per launch, and one JSON line.  Every keyframe holds its code, so the
solver works on the pose and scale rows only: blocks of Bs = 7 rows (padded to Bp = 8) out of the B = 7 + CS of the packed
buffer (sage_window_solver_block_size).  profiles/loop_graph_bench.txt has the measurement.

    python scripts/loop_graph_bench.py [--keyframes 512 --height 64 --width 80 --points 128 --no-loops --out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOPS = [(0, 511), (2, 509), (1, 510), (0, 256), (100, 130)]          # BASELINE config 5


def lm_cfg(capi):
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    return cfg


def lm_step_ms(capi, win, cycles=8, restart=5):
    cfg = lm_cfg(capi)
    st = capi.SageLmState()
    steady = []
    for c in range(cycles + 2):
        win.reset()
        st.iters = 0; st.damp = float(cfg.init_damp)
        _, sec = win.lm_run_timed(st, cfg, restart)
        if c >= 2:                                   # two warm-up cycles
            steady += [float(s) for s in sec[1:]]    # (the first iteration of a cycle forms the system from scratch)
    return 1e3 * float(np.median(steady)), len(steady)


def phase_split_ms(capi, win, cycles=4, restart=5):
    win.set_profiling(1)
    win.phase_time()
    for which in (4, 5):
        win.kernel_time(which)
    cfg = lm_cfg(capi)
    st = capi.SageLmState()
    for _ in range(cycles):
        win.reset()
        st.iters = 0; st.damp = float(cfg.init_damp)
        win.lm_run(st, cfg, restart)
    ms, n = win.phase_time()
    kern = []
    for which in (4, 5):
        t, launches = win.kernel_time(which)
        kern.append(1e3 * t / max(launches, 1))
    dense_launches = sum(win.kernel_time(which)[1] for which in range(4))
    win.set_profiling(0)
    return {k: v / max(n, 1) for k, v in ms.items()}, kern, dense_launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=512)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--no-loops", action="store_true", help="without the loop closures of BASELINE config 5")
    ap.add_argument("--out", default=None, help="also write the text report here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    K = args.keyframes
    w = synth.make_window(K=K, H=args.height, W=args.width, FS=16, CS=32, L=4, n_samples=3072, seed=0, loop_radius=0.12)
    links = list(w.links)
    if not args.no_loops:
        links += [l for l in LOOPS if l[1] < K and l not in links]
    terms = []
    for l, (a, b) in enumerate(links):
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            t = synth.make_loop_mg_exact(w, k0, k1, args.points, 2 * l + d)
            t.update(edge=2 * l + d, weight=5.0, loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
            terms.append(t)
    holds = {k: capi.SAGE_HOLD_CODE for k in range(K)}
    holds[0] = capi.SAGE_HOLD_POSE | capi.SAGE_HOLD_CODE | capi.SAGE_HOLD_SCALE
    win = capi.Window(dataclasses.replace(w, links=[]), keypoint_links=links, keypoint_terms=terms, holds=holds)
    Bs = win.Bs
    Bp = 8 if Bs <= 8 else 24 if Bs <= 24 else 40                     # block_solver.h: padded_block
    step_ms, n_steps = lm_step_ms(capi, win)
    phases, (lin_us, err_us), dense_launches = phase_split_ms(capi, win)
    st = capi.SageLmState(); st.damp = 1e-3
    win.reset()
    tr = win.lm_run(st, lm_cfg(capi), 6)
    win.close()
    other = step_ms - sum(phases.values())
    lines = [f"loop_graph_bench: K {K}, {args.height} x {args.width}, CS 32 (B = {win.B}, solver rows Bs = {Bs}, padded Bp = {Bp}), {len(links)} keypoint links "
             f"({'no' if args.no_loops else len(links) - len(w.links)} loop closures), {len(terms)} loop-MG terms of {args.points} "
             f"points, all codes and keyframe 0 held; device {torch.cuda.get_device_name(0)}",
             f"LM step                                    {step_ms:8.3f} ms   (median of {n_steps} steady iterations)",
             f"  linearize (one launch for all terms + assembly) {phases['linearize']:8.3f} ms",
             f"  all-reduce                                      {phases['allreduce']:8.3f} ms",
             f"  solve (scatter + host factorisation + retract)  {phases['solve']:8.3f} ms",
             f"  error pass                                      {phases['error_pass']:8.3f} ms",
             f"  host time with the device idle                  {other:8.3f} ms",
             f"batched kernel: linearize {lin_us:7.1f} us, error pass {err_us:7.1f} us per launch (all terms); "
             f"dense kernel launches: {dense_launches}",
             f"six LM steps from the synthetic start: error {tr[0, 0]:.4f} -> {st.error:.3e}, {int(tr[:, 2].sum())} accepted"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(dict(keyframes=K, links=len(links), terms=len(terms), points=args.points, B=win.B, Bs=Bs, Bp=Bp, step_ms=step_ms, phases_ms=phases,
                          kernel_linearize_us=lin_us, kernel_error_us=err_us, dense_launches=dense_launches)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
