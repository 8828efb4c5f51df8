#!/usr/bin/env python3
"""What batching the matched-keypoint terms buys, on the headline window (K = 64, 128 x 160 x 16, CS 32, 372 directed
edges), one term of 128 keypoints per directed edge, in ONE process:

  (a) LM step of the window without terms           (median of the steady iterations of sage_window_lm_run_timed)
  (b) the same with the terms                       (sage_window_add_keypoint_term: one launch per pass for all of them)
  (c) one pass of the per-edge operator over the same terms (median of five passes after one warm-up pass): what a caller
      had to do before the window took such terms -- two launches and a blocking synchronise per term

for reprojection terms and again for match-geometry terms, plus the batched kernel's own time (sage_window_get_kernel_time
4 / 5).  The requirement it checks: (b) - (a) <= (c) / 10.  Prints a text report and one JSON line; exit status 1 when the
requirement is missed.

    python scripts/keypoint_window_bench.py [--keyframes 64 --height 128 --width 160 --points 128 --out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lm_step_ms(capi, win, cycles=8, restart=5):
    cfg = capi.lm_config_default()
    cfg.max_inner_evals = 1
    st = capi.SageLmState()
    steady = []
    for c in range(cycles + 2):
        win.reset()
        st.iters = 0; st.damp = float(cfg.init_damp)
        _, sec = win.lm_run_timed(st, cfg, restart)
        if c >= 2:                                   # two warm-up cycles
            steady += [float(s) for s in sec[1:]]    # (the first iteration of a cycle forms the system from scratch)
    return 1e3 * float(np.median(steady))


def kernel_us(win, passes=20):
    import torch
    win.set_profiling(1)
    for which in (4, 5):
        win.kernel_time(which)
    for _ in range(passes):
        win.linearize(); win.error(0)
    torch.cuda.synchronize()
    out = []
    for which in (4, 5):
        ms, n = win.kernel_time(which)
        out.append(1e3 * ms / max(n, 1))
    win.set_profiling(0)
    return out


def per_edge_pass_ms(capi, torch, w, win, terms, kind):
    """the per-edge operators over the same terms at the window's initial variables; every array is on the device beforehand"""
    ws = capi.Workspace()
    cam = win.pyr.cam[0]
    prepared = []
    for t in terms:
        a, b = w.links[t["edge"] // 2]
        k0, k1 = (a, b) if t["edge"] % 2 == 0 else (b, a)
        f0, f1 = w.keyframes[k0], w.keyframes[k1]
        from sage_slam_amd import synth
        R10, t10 = synth.relative_pose(f0.R, f0.t, f1.R, f1.t)
        dev = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
        p = dict(R10=dev(R10), t10=dev(t10), R0=dev(f0.R), t0=dev(f0.t), R1=dev(f1.R), t1=dev(f1.t), code0=dev(f0.code),
                 code1=dev(f1.code), loc0=dev(t["loc0"], np.int32), homo0=dev(t["homo0"]), k0=k0, k1=k1, t=t)
        if kind == "reprojection":
            p["m2d"] = dev(t["matched_2d"])
        else:
            p["loc1"] = dev(t["loc1"], np.int32); p["homo1"] = dev(t["homo1"])
        prepared.append(p)
    torch.cuda.synchronize()

    def one_pass():
        for p in prepared:
            t, d0, d1 = p["t"], win.kfs[p["k0"]], win.kfs[p["k1"]]
            f0, f1 = w.keyframes[p["k0"]], w.keyframes[p["k1"]]
            if kind == "reprojection":
                capi.reprojection_jac_error(ws, p["R10"], p["t10"], p["R0"], p["t0"], p["R1"], p["t1"], d0.bias, d0.basis,
                                            p["code0"], p["loc0"], p["homo0"], p["m2d"], f0.scale, cam, w.eps,
                                            t["loss_param"], t["weight"], w.CS)
            else:
                capi.match_geometry(ws, t["loss"], True, p["R10"], p["t10"], p["R0"], p["t0"], p["R1"], p["t1"], d0.bias,
                                    d1.bias, d0.basis, d1.basis, p["code0"], p["code1"], p["homo0"], p["homo1"], p["loc0"],
                                    p["loc1"], f0.scale, f1.scale, t["loss_param"], t["weight"], w.CS)

    one_pass()
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    ws.close()
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--points", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the text report here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    w = synth.make_window(K=args.keyframes, H=args.height, W=args.width, FS=16, CS=32, L=4, seed=0)
    n_edges = 2 * len(w.links)

    def terms_of(kind):
        out = []
        for e in range(n_edges):
            a, b = w.links[e // 2]
            k0, k1 = (a, b) if e % 2 == 0 else (b, a)
            if kind == "reprojection":
                t = synth.make_reprojection_matches(w, k0, k1, args.points, e)
                t.update(edge=e, weight=5.0, loss_param=0.1 * w.W * w.W)          # demo/main.cpp:254-278
            else:
                t = synth.make_match_geometry_matches(w, k0, k1, args.points, e)
                t.update(edge=e, weight=5.0, loss="fair",
                         loss_param=float(0.1 * np.mean(np.square(w.keyframes[k0].bias, dtype=np.float64))))
            out.append(t)
        return out

    lines = [f"keypoint_window_bench: K {args.keyframes}, {args.height} x {args.width} x 16, CS 32, {n_edges} directed edges, "
             f"one term of {args.points} keypoints per edge; device {torch.cuda.get_device_name(0)}"]
    result, ok = {"edges": n_edges, "points": args.points}, True
    dense = capi.Window(w)
    a_ms = lm_step_ms(capi, dense)
    dense.close()
    lines.append(f"(a) LM step without terms                      {a_ms:8.3f} ms")
    result["a_ms"] = a_ms
    for kind in ("reprojection", "match_geometry"):
        terms = terms_of(kind)
        win = capi.Window(w, keypoint_terms=terms)
        b_ms = lm_step_ms(capi, win)
        lin_us, err_us = kernel_us(win)
        win.reset()
        c_ms = per_edge_pass_ms(capi, torch, w, win, terms, kind)
        win.close()
        passed = (b_ms - a_ms) <= c_ms / 10.0
        ok = ok and passed
        lines += [f"[{kind}]",
                  f"(b) LM step with {n_edges} terms                    {b_ms:8.3f} ms   (b) - (a) = {b_ms - a_ms:+.3f} ms",
                  f"    batched kernel: linearize {lin_us:7.1f} us, error pass {err_us:7.1f} us per launch (all terms)",
                  f"(c) one pass of the per-edge operator, {n_edges} calls {c_ms:8.3f} ms   (c) / 10 = {c_ms / 10:.3f} ms",
                  f"    (b) - (a) <= (c) / 10: {'yes' if passed else 'NO'}"]
        result[kind] = dict(b_ms=b_ms, c_ms=c_ms, kernel_linearize_us=lin_us, kernel_error_us=err_us, passed=passed)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
