#!/usr/bin/env python3
"""A window's keypoint and graph terms served from the gtsam factor cache (sage_window_prepass with terms,
sage_window_prepare_factors / _device, sage_window_keypoint_factor / sage_window_graph_factor), in one process.

(a) The headline window (K = 64, 128 x 160, CS 32) with one match-geometry term of 512 keypoints on every directed edge:
    prepass         one sage_window_prepass with jacobians at new values (the linearize and the copy of every result)
    device          sage_window_prepare_factors_device: dense factors and terms, one launch per type / group, one wait
    host_16         sage_window_prepare_factors(1, 16)
    read            sage_window_keypoint_factor(.., 1, ..) of every term after a preparation: blocks are cut only
    read_lazy       the same without a preparation: every read projects its 78 x 78 on the calling thread
    baseline        what a caller has without the cache: sage_window_get_keypoint_term + sage_nearest_psd per term
    Before every timed preparation the previous one is dropped by an untimed sage_window_prepare_factors with mode 0.
(b) The K = 512 loop graphs of scripts/loop_graph_bench.py --terms both (loop-MG terms; relative-pose-scale terms and scale
    priors): the D = 14 projection alone -- sage_factor_psd_batch on the group's systems between two HIP events on the
    workspace's stream (the projection kernel and the one-lane ticket kernel behind it) -- and per term next to the host's
    sage_nearest_psd on one thread and sage_window_prepare_factors on 16.
Wall-clock times are the median [min max] of RUNS runs after WARMUP unrecorded ones.  No time here is a pass criterion.

    python scripts/term_factor_bench.py [--out FILE] [--skip-graph]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

WARMUP, RUNS = 3, 10


def timed(fn, before=None, runs=RUNS, warmup=WARMUP):
    ms = []
    for i in range(warmup + runs):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), "%.3f [%.3f %.3f]" % (float(np.median(ms)), min(ms), max(ms))


def values_of(w, bump=0.0):
    poses = np.stack([np.concatenate([np.asarray(k.R, np.float32).reshape(-1), np.asarray(k.t, np.float32).reshape(-1)])
                      for k in w.keyframes])
    poses[:, 9:] += np.float32(bump)
    codes = np.stack([np.asarray(k.code, np.float32).reshape(-1) for k in w.keyframes])
    scales = np.array([k.scale for k in w.keyframes], np.float32)
    return poses, codes, scales


def bench_a(say, torch, capi, synth):
    K, CS, N = 64, 32, 512
    w = synth.make_window(K=K, H=128, W=160, FS=16, CS=CS, L=4, seed=0)
    terms = []
    for l, (a, b) in enumerate(w.links):
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            t = synth.make_match_geometry_matches(w, k0, k1, N, 2000 + 2 * l + d)
            t.update(edge=2 * l + d, weight=5.0, loss="fair",
                     loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
            terms.append(t)
    win = capi.Window(w, keypoint_terms=terms)
    nt, ne = len(terms), 2 * len(w.links)
    say("(a) K = %d, 128 x 160, CS = %d: %d + %d dense factors (D = %d, %d) and %d match-geometry terms of %d keypoints (D = %d)"
        % (K, CS, ne, ne, 13 + CS, 14 + 2 * CS, nt, N, 14 + 2 * CS))
    state = {"i": 0}

    def prepass():
        state["i"] += 1
        assert win.prepass(*values_of(w, 1e-4 * state["i"]), True)

    say("  prepass       %s" % timed(prepass)[1])
    drop = lambda: win.prepare_factors(0, 1)
    drop()
    worst = win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 3
    say("  worst record: status %d, sweeps %d, bump rounds %d" % (worst.status, worst.sweeps, worst.bump_rounds))
    dev, s = timed(win.prepare_factors_device, drop)
    say("  device        %s   (%.2f us per factor, dense and terms)" % (s, 1e3 * dev / (2 * ne + nt)))
    host, s = timed(lambda: win.prepare_factors(1, 16), drop)
    say("  host_16       %s   (%.2f us per factor)" % (s, 1e3 * host / (2 * ne + nt)))
    read_all = lambda: [win.keypoint_factor(i, 1) for i in range(nt)]
    win.prepare_factors_device()
    rd, s = timed(read_all)
    say("  read          %s   (%.2f us per term)" % (s, 1e3 * rd / nt))
    drop()
    lazy, s = timed(read_all, runs=3, warmup=1)
    say("  read_lazy     %s   (%.2f us per term)" % (s, 1e3 * lazy / nt))

    def baseline():
        for i in range(nt):
            capi.nearest_psd(win.get_keypoint_term(i)["AtA"].astype(np.float64))

    base, s = timed(baseline, runs=3, warmup=1)
    say("  baseline      %s   (%.2f us per term: get_keypoint_term + nearest_psd, no dense factor)" % (s, 1e3 * base / nt))
    win.close()


def bench_b(say, torch, capi, synth):
    import loop_graph_bench as lg
    K = 512
    w = synth.make_window(K=K, H=64, W=80, FS=16, CS=32, L=4, n_samples=3072, seed=0, loop_radius=0.12)
    local = list(w.links)
    loops = [l for l in lg.LOOPS if l[1] < K and l not in local]
    stream = torch.cuda.Stream()
    ws = capi.Workspace(stream)
    for name in ("loop_mg", "graph"):
        if name == "loop_mg":
            win, n, what = lg.build_loop_mg(capi, synth, w, local + loops, 128)
            get = win.get_keypoint_term
        else:
            win, n, what = lg.build_graph(capi, synth, w, local, loops)
            get = win.get_graph_term
        poses, codes, scales = [], [], []
        for k in range(win.K):
            p, c, s = win.get_keyframe(k)
            poses.append(p); codes.append(c); scales.append(s)
        assert win.prepass(np.stack(poses), np.stack(codes), np.array(scales, np.float32), True)
        mats = np.stack([get(i)["AtA"] for i in range(n)])
        A = torch.from_numpy(mats).cuda()
        torch.cuda.synchronize()
        us = []
        for i in range(WARMUP + RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            capi.factor_psd_batch(ws, A)
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                us.append(1e3 * e0.elapsed_time(e1))
        ev = float(np.median(us))
        one = mats.astype(np.float64)
        h1, _ = timed(lambda: [capi.nearest_psd(M) for M in one], runs=3, warmup=1)
        drop = lambda: win.prepare_factors(0, 1)
        h16, _ = timed(lambda: win.prepare_factors(1, 16), drop)
        dv, _ = timed(win.prepare_factors_device, drop)
        drop()
        worst = win.prepare_factors_device()
        launches = win.prepare_factors_device_launches()
        say("(b) K = %d loop graph, %s: %d terms, D = 14" % (K, what, n))
        say("  D = 14 launch between HIP events   %.1f us [%.1f %.1f]   %.3f us per term" % (ev, min(us), max(us), ev / n))
        say("  sage_window_prepare_factors_device %.3f ms wall (%d launch, copies, one wait)   %.3f us per term; worst record: "
            "status %d, sweeps %d, bump rounds %d" % (dv, launches, 1e3 * dv / n, worst.status, worst.sweeps, worst.bump_rounds))
        say("  host: sage_nearest_psd on one thread %.3f ms   %.3f us per term; sage_window_prepare_factors(1, 16) %.3f ms   "
            "%.3f us per term" % (h1, 1e3 * h1 / n, h16, 1e3 * h16 / n))
        win.close()
    ws.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-graph", action="store_true", help="bench (a) only")
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                             # (kept current: a later step may be cut short)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say("device: %s; host threads available to this process: %d" % (torch.cuda.get_device_name(0), len(os.sched_getaffinity(0))))
    say("ms per call, median [min max] of %d runs after %d warm-up runs (read_lazy, baseline, one-thread host: 3 after 1)" % (RUNS, WARMUP))
    bench_a(say, torch, capi, synth)
    if not a.skip_graph:
        bench_b(say, torch, capi, synth)


if __name__ == "__main__":
    main()
