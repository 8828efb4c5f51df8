#!/usr/bin/env python3
"""The projection of a window's factors to their nearest PSD (psd_mode 1), on the device and on host threads, in one
process: the headline window (K = 64, CS 32: 372 photometric 45 x 45 and 372 geometric 78 x 78 factors) and K = 16 at CS 16
(90 of 29 x 29, 90 of 46 x 46).

Per window, after one prepass with jacobians, each of these is run 5 times unrecorded and 20 times timed (wall clock around
the call, median [min max] in ms); before every run the preparation is dropped by an untimed sage_window_prepare_factors
with mode 0, so every run projects every factor:
  device          sage_window_prepare_factors_device: one launch per factor type, the copies of the projected matrices
                  and records to the host, one wait
  host_16         sage_window_prepare_factors(1, 16)
  host_default    sage_window_prepare_factors(1, 0): a quarter of the host's hardware threads, at most 64
  kernel_photo / kernel_geo   sage_factor_psd_batch on the same per-edge systems held in device tensors: the projection
                  kernel, the ticket, nothing copied back but the records
Then the parity of sage_factor_psd_batch with sage_nearest_psd on the input families of tests/psd_ref.py: per family and D
the worst ||C_dev - host||_F as a fraction of the bar 32 D 2^-52 ||B||_F, with the most sweeps and bump rounds seen.
No time here is a pass criterion.  Prints text lines; --out also writes them to a file.

    python scripts/psd_project_bench.py [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, RUNS = 5, 20


def timed(fn, before=None):
    ms = []
    for i in range(WARMUP + RUNS):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            ms.append(1e3 * (time.perf_counter() - t0))
    return "%.3f [%.3f %.3f]" % (float(np.median(ms)), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    from tests import psd_ref
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; host threads available to this process: %d" % (torch.cuda.get_device_name(0), len(os.sched_getaffinity(0))))
    say("ms per call, median [min max] of %d runs after %d warm-up runs" % (RUNS, WARMUP))
    ws = capi.Workspace()
    for K, CS in ((64, 32), (16, 16)):
        w = synth.make_window(K=K, H=128, W=160, FS=16, CS=CS, L=4, seed=0)
        win = capi.Window(w)
        poses = np.stack([np.concatenate([np.asarray(k.R, np.float32).reshape(-1), np.asarray(k.t, np.float32).reshape(-1)])
                          for k in w.keyframes])
        codes = np.stack([np.asarray(k.code, np.float32).reshape(-1) for k in w.keyframes])
        scales = np.array([k.scale for k in w.keyframes], np.float32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert win.prepass(poses, codes, scales, True)
        t_pre = 1e3 * (time.perf_counter() - t0)
        ne = 2 * len(w.links)
        drop = lambda: win.prepare_factors(0, 1)
        say("K = %d, CS = %d: %d + %d factors (D = %d, %d); first prepass with jacobians %.2f ms" %
            (K, CS, ne, ne, 13 + CS, 14 + 2 * CS, t_pre))
        worst = win.prepare_factors_device()
        assert win.prepare_factors_device_launches() == 2
        say("  worst record: status %d, sweeps %d, bump rounds %d" % (worst.status, worst.sweeps, worst.bump_rounds))
        say("  device        %s" % timed(win.prepare_factors_device, drop))
        say("  host_16       %s" % timed(lambda: win.prepare_factors(1, 16), drop))
        say("  host_default  %s" % timed(lambda: win.prepare_factors(1, 0), drop))
        for t, name in ((0, "kernel_photo"), (1, "kernel_geo  ")):
            A = torch.from_numpy(np.stack([win.get_edge(t, e)["AtA"] for e in range(ne)])).cuda()
            say("  %s  %s" % (name, timed(lambda: capi.factor_psd_batch(ws, A))))
        win.close()
    say("parity with sage_nearest_psd, worst ||C_dev - host||_F / (32 D 2^-52 ||B||_F) per family; most sweeps, most bump rounds")
    for D in psd_ref.DIMS:
        cases = psd_ref.cases(D)
        mats = np.stack([M for _, _, M in cases])
        Cd, stats = capi.factor_psd_batch(ws, torch.from_numpy(mats).cuda())
        Cd = Cd.cpu().numpy()
        worst = {}
        for i, (name, seed, M) in enumerate(cases):
            bar = 32 * D * psd_ref.EPS * np.linalg.norm(psd_ref.symmetrised(M))
            err = np.linalg.norm(Cd[i] - capi.nearest_psd(M.astype(np.float64)))
            worst[name] = max(worst.get(name, 0.0), err / bar if bar > 0 else float(err > 0))
        say("  D = %2d: %s; sweeps %d, bump rounds %d" % (D, ", ".join("%s %.3g" % kv for kv in worst.items()),
                                                         max(s.sweeps for s in stats), max(s.bump_rounds for s in stats)))
    ws.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
