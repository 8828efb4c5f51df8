#!/usr/bin/env python3
"""The dogleg step next to the LM step, measured on the headline window (K = 64 at 128 x 160, dense factors) and on the K = 512
loop-closure graphs of scripts/loop_graph_bench.py (loop-MG keypoint terms; relative-pose-scale terms), in one process:

  * ms per iteration: sage_window_dogleg_step (gtsam's defaults: radius 1.0, ONE_STEP_PER_ITERATION) and sage_window_lm_step
    (one evaluation per step, as bench.py runs it), each the median host time of the steady iterations after a reset -- an
    iteration returns once its accept / reject decision is taken, so the clock stops behind a wait on the device;
  * ms per ADDITIONAL evaluation of the same iteration, what a rejection costs: for LM a solve at another damping, the error
    pass and the read of its total; for the dogleg the candidate kernel for another (a, b), the error pass and the read.  Both
    are timed through the step's own primitives on a system that is already linearized (and, for the dogleg, solved) -- the
    synthetic windows reject too rarely to time rejections where they fall; how often they do is printed;
  * the product kernels (both, until the dots are seen on the host) and the candidate kernel by device events.

    python scripts/dogleg_bench.py [--keyframes 64 --height 128 --width 160 --loop-keyframes 512 --skip-loop --out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def median_ms(samples):
    return 1e3 * float(np.median(samples)), len(samples)


def lm_iteration_ms(capi, win, cycles=6, restart=5):
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    st = capi.SageLmState()
    steady, accepted = [], 0
    for c in range(cycles + 2):
        win.reset()
        st.iters = 0; st.damp = float(cfg.init_damp)
        tr, sec = win.lm_run_timed(st, cfg, restart)
        if c >= 2:                                   # two warm-up cycles
            steady += [float(s) for s in sec[1:]]    # (the first iteration of a cycle forms the system from scratch)
            accepted += int(tr[1:, 2].sum())
    return median_ms(steady) + (accepted,)


def dogleg_iteration_ms(capi, win, cycles=6, restart=5, init_delta=None):
    """-> (median ms, iterations, accepted, evaluations, last trace row) of the steady iterations"""
    cfg = capi.dogleg_config_default()
    if init_delta is not None:
        cfg.init_delta = init_delta
    steady, accepted, evals, last = [], 0, 0, None
    for c in range(cycles + 2):
        win.reset()
        st = capi.SageDoglegState()
        for i in range(restart):
            t0 = time.perf_counter()
            win.dogleg_step(st, cfg)
            dt = time.perf_counter() - t0
            if c >= 2 and i >= 1:
                steady.append(dt)
                accepted += st.accepted
                evals += st.evals
            last = (st.error, st.candidate_error, st.delta, st.rho, st.region)
    return median_ms(steady) + (accepted, evals, last)


def extra_evaluation_ms(capi, torch, win, reps=30):
    """what one more evaluation of the same iteration costs, through the primitives: (LM ms, dogleg ms)"""
    win.reset()
    win.linearize()
    lm, dl = [], []
    damp = 1e-3
    for i in range(reps + 5):
        damp *= 1.5
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        win.solve(damp, want_norm=False)
        win.error(1)
        win.total_error(False)
        if i >= 5:
            lm.append(time.perf_counter() - t0)
    win.solve(0.0, want_norm=False)
    dots = win.dogleg_products()
    radius = np.sqrt(dots[2])
    for i in range(reps + 5):
        radius *= 0.9                                # a smaller radius every time, as a rejection asks for
        rc, a, b, _ = capi.dogleg_point(radius, *dots[:4])
        assert rc == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        win.dogleg_candidate(a, b)
        win.error(1)
        win.total_error(False)
        if i >= 5:
            dl.append(time.perf_counter() - t0)
    return median_ms(lm)[0], median_ms(dl)[0]


def kernel_times_us(capi, torch, win, reps=50):
    """(products, candidate) by device events around the calls, median of `reps`"""
    win.reset()
    win.linearize()
    win.solve(0.0, want_norm=False)
    dots = win.dogleg_products()
    rc, a, b, _ = capi.dogleg_point(0.5 * np.sqrt(dots[2]), *dots[:4])
    out = []
    for call in (win.dogleg_products, lambda: win.dogleg_candidate(a, b)):
        ts = []
        for _ in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out.append(1e3 * float(np.median(ts[5:])))
    return out[0], out[1]


def measure(capi, torch, win, title):
    lm_ms, lm_n, lm_acc = lm_iteration_ms(capi, win)
    dl_ms, dl_n, dl_acc, dl_evals, last = dogleg_iteration_ms(capi, win)
    big_ms, big_n, big_acc, big_evals, _ = dogleg_iteration_ms(capi, win, init_delta=1e6)
    lm_extra, dl_extra = extra_evaluation_ms(capi, torch, win)
    prod_us, cand_us = kernel_times_us(capi, torch, win)
    lines = [title,
             f"  LM iteration      (one evaluation)          {lm_ms:8.3f} ms   median of {lm_n}, {lm_acc} accepted",
             f"  dogleg iteration  (radius 1.0)              {dl_ms:8.3f} ms   median of {dl_n}, {dl_acc} accepted, {dl_evals} evaluations",
             f"  dogleg iteration  (radius 1e6: GN first)    {big_ms:8.3f} ms   median of {big_n}, {big_acc} accepted, {big_evals} evaluations",
             f"  one more evaluation, LM     (solve + error pass + read)      {lm_extra:8.3f} ms",
             f"  one more evaluation, dogleg (candidate + error pass + read)  {dl_extra:8.3f} ms",
             f"  product kernels until the dots are seen {prod_us:7.1f} us, candidate kernel {cand_us:7.1f} us (device events)",
             f"  last dogleg iteration: error {last[0]:.6g} -> {last[1]:.6g}, radius {last[2]:.4g}, rho {last[3]:.3f}, region {last[4]}"]
    res = dict(lm_ms=lm_ms, dogleg_ms=dl_ms, dogleg_gn_first_ms=big_ms, lm_extra_eval_ms=lm_extra, dogleg_extra_eval_ms=dl_extra,
               products_us=prod_us, candidate_us=cand_us, dogleg_evals=dl_evals, dogleg_iters=dl_n)
    return lines, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--loop-keyframes", type=int, default=512)
    ap.add_argument("--skip-loop", action="store_true", help="the headline window only")
    ap.add_argument("--out", default=None, help="also write the text report here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "dogleg_bench.py measures on the GPU"
    dev = torch.cuda.get_device_name(0)
    lines, out = [f"dogleg_bench: device {dev}; host times are medians of steady iterations, see scripts/dogleg_bench.py"], {}
    w = synth.make_window(K=args.keyframes, H=args.height, W=args.width, FS=16, CS=32, L=4, seed=0)
    win = capi.Window(w)
    ls, out["headline"] = measure(capi, torch, win, f"headline window: K {args.keyframes}, {args.height} x {args.width}, CS 32, "
                                                    f"{len(w.links)} dense links")
    win.close()
    lines += [""] + ls
    if not args.skip_loop:
        import loop_graph_bench as lg
        K = args.loop_keyframes
        wl = synth.make_window(K=K, H=64, W=80, FS=16, CS=32, L=4, n_samples=3072, seed=0, loop_radius=0.12)
        local = list(wl.links)
        loops = [l for l in lg.LOOPS if l[1] < K and l not in local]
        for mode in ("loop_mg", "graph"):
            if mode == "loop_mg":
                win, n, what = lg.build_loop_mg(capi, synth, wl, local + loops, 128)
            else:
                win, n, what = lg.build_graph(capi, synth, wl, local, loops)
            ls, out[mode] = measure(capi, torch, win, f"loop graph ({mode}): K {K}, {len(local + loops)} keypoint links, {what}; "
                                                      f"solver rows {win.Bs} of {win.B}")
            win.close()
            lines += [""] + ls
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
