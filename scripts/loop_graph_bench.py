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

--terms graph times the graph the reference actually solves after an accepted loop (DeepFactors::LoopClosurePoseScaleEstimate)
on the same keyframes and links instead: no keypoint at all, two relative-pose-scale terms per link (local links on target, the
loop closures on the true relative pose of a drifted start), a weight-100 scale prior on keyframe 0, two on the first loop's
keyframes (synth.make_pose_graph; sage_window_add_graph_term).  --terms both runs the two one after the other.

    python scripts/loop_graph_bench.py [--keyframes 512 --height 64 --width 80 --points 128 --no-loops --terms loop_mg|graph|both
                                        --out FILE]
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


def phase_split_ms(capi, win, cycles=4, restart=5, slots=(4, 5)):
    """slots: the kernel-time slots of the terms' batched kernel -- (4, 5) keypoint terms, (6, 7) graph terms"""
    win.set_profiling(1)
    win.phase_time()
    for which in slots:
        win.kernel_time(which)
    cfg = lm_cfg(capi)
    st = capi.SageLmState()
    for _ in range(cycles):
        win.reset()
        st.iters = 0; st.damp = float(cfg.init_damp)
        win.lm_run(st, cfg, restart)
    ms, n = win.phase_time()
    kern = []
    for which in slots:
        t, launches = win.kernel_time(which)
        kern.append(1e3 * t / max(launches, 1))
    dense_launches = sum(win.kernel_time(which)[1] for which in range(4))
    win.set_profiling(0)
    return {k: v / max(n, 1) for k, v in ms.items()}, kern, dense_launches


def build_loop_mg(capi, synth, w, links, points):
    terms = []
    for l, (a, b) in enumerate(links):
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            t = synth.make_loop_mg_exact(w, k0, k1, points, 2 * l + d)
            t.update(edge=2 * l + d, weight=5.0, loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
            terms.append(t)
    holds = {k: capi.SAGE_HOLD_CODE for k in range(len(w.keyframes))}
    holds[0] = capi.SAGE_HOLD_POSE | capi.SAGE_HOLD_CODE | capi.SAGE_HOLD_SCALE
    win = capi.Window(dataclasses.replace(w, links=[]), keypoint_links=links, keypoint_terms=terms, holds=holds)
    return win, len(terms), f"{len(terms)} loop-MG terms of {points} points, all codes and keyframe 0 held"


def build_graph(capi, synth, w, local_links, loops):
    wg, links, terms, holds = synth.make_pose_graph(w, local_links, loops=loops, drift=0.002, seed=0)
    win = capi.Window(wg, keypoint_links=links, graph_terms=terms, holds=holds, code_prior_weight=0.0, scale_prior_weight=0.0,
                      pose_prior_weight=0.0)
    n_prior = sum(t["kind"] == "scale_prior" for t in terms)
    return win, len(terms), (f"{len(terms) - n_prior} relative-pose-scale terms + {n_prior} scale priors (no keypoint), all codes "
                             "and keyframe 0's pose held")


def report(capi, torch, win, K, args, links, n_loops, what, slots, kernel_name):
    Bs = win.Bs
    Bp = 8 if Bs <= 8 else 24 if Bs <= 24 else 40                     # block_solver.h: padded_block
    step_ms, n_steps = lm_step_ms(capi, win)
    phases, (lin_us, err_us), dense_launches = phase_split_ms(capi, win, slots=slots)
    st = capi.SageLmState(); st.damp = 1e-3
    win.reset()
    tr = win.lm_run(st, lm_cfg(capi), 6)
    other = step_ms - sum(phases.values())
    lines = [f"loop_graph_bench: K {K}, {args.height} x {args.width}, CS 32 (B = {win.B}, solver rows Bs = {Bs}, padded Bp = {Bp}), {len(links)} keypoint links "
             f"({n_loops or 'no'} loop closures), {what}; device {torch.cuda.get_device_name(0)}",
             f"LM step                                    {step_ms:8.3f} ms   (median of {n_steps} steady iterations)",
             f"  linearize (one launch for all terms + assembly) {phases['linearize']:8.3f} ms",
             f"  all-reduce                                      {phases['allreduce']:8.3f} ms",
             f"  solve (scatter + host factorisation + retract)  {phases['solve']:8.3f} ms",
             f"  error pass                                      {phases['error_pass']:8.3f} ms",
             f"  host time with the device idle                  {other:8.3f} ms",
             f"{kernel_name}: linearize {lin_us:7.1f} us, error pass {err_us:7.1f} us per launch (all terms); "
             f"dense kernel launches: {dense_launches}",
             f"six LM steps from the synthetic start: error {tr[0, 0]:.4f} -> {st.error:.3e}, {int(tr[:, 2].sum())} accepted"]
    result = dict(B=win.B, Bs=Bs, Bp=Bp, step_ms=step_ms, phases_ms=phases, kernel_linearize_us=lin_us, kernel_error_us=err_us,
                  dense_launches=dense_launches)
    return lines, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=512)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--no-loops", action="store_true", help="without the loop closures of BASELINE config 5")
    ap.add_argument("--terms", choices=("loop_mg", "graph", "both"), default="loop_mg",
                    help="loop_mg: the keypoint graph of LoopClosurePoseScaleMGEstimate; graph: the relative-pose-scale graph of "
                         "LoopClosurePoseScaleEstimate; both: one after the other")
    ap.add_argument("--out", default=None, help="also write the text report here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    K = args.keyframes
    w = synth.make_window(K=K, H=args.height, W=args.width, FS=16, CS=32, L=4, n_samples=3072, seed=0, loop_radius=0.12)
    local = list(w.links)
    loops = [] if args.no_loops else [l for l in LOOPS if l[1] < K and l not in local]
    links = local + loops
    lines, out = [], dict(keyframes=K, links=len(links), points=args.points)
    for mode in (("loop_mg", "graph") if args.terms == "both" else (args.terms,)):
        if mode == "loop_mg":
            win, n, what = build_loop_mg(capi, synth, w, links, args.points)
            ls, res = report(capi, torch, win, K, args, links, len(loops), what, (4, 5), "batched kernel")
        else:
            win, n, what = build_graph(capi, synth, w, local, loops)
            ls, res = report(capi, torch, win, K, args, links, len(loops), what, (6, 7), "graph-term kernel")
        win.close()
        res["terms"] = n
        lines += ([""] if lines else []) + ls
        if args.terms == "both":
            out[mode] = res
        else:
            out.update(res)
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
