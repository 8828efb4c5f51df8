#!/usr/bin/env python3
"""What a marginal prior costs and what carrying one buys, one JSON line per measurement (medians taken in this one process):

  * term: prior_eval_kernel and prior_add_kernel per linearize (HIP events, sage_window_get_kernel_time slots 8 / 9) for a
    prior over m = 3 and m = 8 keyframes at CS = 32 on a 16-keyframe 128 x 160 x 16 window, next to the wall time of an LM step
    of the same window with and without the prior (the two windows alternate step by step).
  * marginalize: sage_window_marginalize per call on the 17-keyframe window those priors come from (separator 3 and 8).
  * sliding: 20 slides of a 16-keyframe window over 35 keyframes, a few LM steps per window -- with the prior of the keyframe
    that leaves carried into the next window, with nothing carried (every window anchors its own first keyframe), and one
    batch over all 35 keyframes.  Reported: the error of the relative poses (k, k + 3) against the truth at the end of each.
    Numbers to report; no threshold applies to them.

    python scripts/marginal_prior_bench.py [--steps 40 --warmup 8 --out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(x, scale=1e3):
    return round(scale * float(np.median(x)), 4)


def sub_scene(w, keep):
    pos = {k: i for i, k in enumerate(keep)}
    return dataclasses.replace(w, keyframes=[w.keyframes[k] for k in keep],
                               links=[(pos[a], pos[b]) for a, b in w.links if a in pos and b in pos])


def term_rows(capi, torch, synth, steps, warmup):
    rows = []
    for m in (3, 8):
        w = synth.make_window(K=17, H=128, W=160, FS=16, CS=32, L=4, seed=0)
        w = dataclasses.replace(w, links=list(w.links) + [(0, k) for k in range(4, m + 1)])   # keyframe 0 linked to 1 .. m
        win = capi.Window(w)
        win.linearize()
        prior = win.marginalize([0])
        sep = prior.get()["keyframes"].tolist()
        assert len(sep) == m
        t_marg = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = win.marginalize([0])
            t_marg.append(time.perf_counter() - t0)
            p.close()
        win.close()
        keep = list(range(1, 17))
        w2 = sub_scene(w, keep)
        with_p = capi.Window(w2, prior_terms=[(prior, [keep.index(k) for k in sep])], scale_prior_weight=0.0, pose_prior_weight=0.0)
        without = capi.Window(w2, keypoint_links=with_p.links[len(w2.links):])
        cfg = capi.lm_config_default()
        st = {id(x): capi.SageLmState() for x in (with_p, without)}
        sec = {id(with_p): [], id(without): []}
        for i in range(warmup + steps):
            for x in (with_p, without):
                x.reset()                                  # the same step every time: from the start variables
                torch.cuda.synchronize()
                st[id(x)] = capi.SageLmState()
                _tr, s = x.lm_run_timed(st[id(x)], cfg, 1)
                torch.cuda.synchronize()
                if i >= warmup:
                    sec[id(x)].append(float(s[0]))
        with_p.set_profiling(1)
        for i in range(steps):
            with_p.linearize(); with_p.error(1)
        ev_ms, ev_n = with_p.kernel_time(8)
        add_ms, add_n = with_p.kernel_time(9)
        with_p.set_profiling(0)
        rows.append(dict(m=m, rows=m * 39, lambda_bytes=(m * 39) ** 2 * 8,
                         prior_eval_kernel_us=round(1e3 * ev_ms / max(1, ev_n), 2), prior_eval_launches=ev_n,
                         prior_add_kernel_us=round(1e3 * add_ms / max(1, add_n), 2), prior_add_launches=add_n,
                         lm_step_with_prior_ms=med(sec[id(with_p)]), lm_step_without_ms=med(sec[id(without)]),
                         marginalize_ms_per_call=med(t_marg[warmup:]), appended_links=len(with_p.links) - len(w2.links)))
        with_p.close(); without.close(); prior.close()
    return rows


def relative_errors(synth, w, est):
    """mean translation / rotation error of the relative poses (k, k + 3) of the estimates against the truth"""
    et, er = [], []
    for k in range(len(w.keyframes) - 3):
        a, b = w.keyframes[k], w.keyframes[k + 3]
        Rt, tt = synth.relative_pose(a.R_true, a.t_true, b.R_true, b.t_true)
        (pa, _ca, _sa), (pb, _cb, _sb) = est[k], est[k + 3]
        Re, te = synth.relative_pose(pa[:9].reshape(3, 3), pa[9:], pb[:9].reshape(3, 3), pb[9:])
        et.append(float(np.linalg.norm(np.asarray(te, np.float64) - tt)))
        er.append(float(np.arccos(np.clip(0.5 * (np.trace(np.asarray(Re, np.float64) @ np.asarray(Rt).T) - 1.0), -1.0, 1.0))))
    return dict(rel_translation_error=float(np.mean(et)), rel_rotation_error_rad=float(np.mean(er)))


def sliding(capi, torch, synth, slides=20, K=16, lm_steps=4):
    n = slides + K - 1
    w = synth.make_window(K=n, H=64, W=80, FS=16, CS=32, L=3, n_samples=1500, seed=3)
    start = [(capi.pack_pose(kf.R, kf.t), np.ascontiguousarray(kf.code, np.float32), float(kf.scale)) for kf in w.keyframes]
    cfg = capi.lm_config_default()
    out = dict(slides=slides, K=K, keyframes=n, lm_steps_per_window=lm_steps, start=relative_errors(synth, w, start))
    for mode in ("prior_carried", "nothing_carried"):
        est = list(start)
        carried = None
        t0 = time.perf_counter()
        for s in range(slides):
            keep = list(range(s, s + K))
            ws = sub_scene(w, keep)
            ws = dataclasses.replace(ws, keyframes=[dataclasses.replace(kf, R=est[k][0][:9].reshape(3, 3), t=est[k][0][9:],
                                                                        code=est[k][1], scale=est[k][2]) for kf, k in zip(ws.keyframes, keep)])
            if carried is not None:
                prior, sep = carried
                win = capi.Window(ws, prior_terms=[(prior, [keep.index(k) for k in sep])], scale_prior_weight=0.0, pose_prior_weight=0.0)
                prior.close()
            else:
                win = capi.Window(ws)
            win.lm_run(capi.SageLmState(), cfg, lm_steps)
            for i, k in enumerate(keep):
                est[k] = win.get_keyframe(i)
            carried = None
            if mode == "prior_carried" and s + 1 < slides:
                win.linearize()
                prior = win.marginalize([0])
                carried = (prior, [keep[i] for i in prior.get()["keyframes"]])
            win.close()
        torch.cuda.synchronize()
        out[mode] = dict(seconds=round(time.perf_counter() - t0, 3), **relative_errors(synth, w, est))
    t0 = time.perf_counter()
    win = capi.Window(w)
    win.lm_run(capi.SageLmState(), cfg, 3 * lm_steps)
    torch.cuda.synchronize()
    out["one_batch"] = dict(seconds=round(time.perf_counter() - t0, 3), lm_steps=3 * lm_steps,
                            **relative_errors(synth, w, [win.get_keyframe(k) for k in range(n)]))
    win.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed repetitions per measurement")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    assert torch.cuda.is_available(), "marginal_prior_bench.py measures on the GPU"
    lines = [dict(bench="marginal_prior", device=torch.cuda.get_device_name(0), method="medians in one process, ways alternating, "
                  "warm-up first; kernels by HIP events on the window's stream", steps=args.steps, warmup=args.warmup)]
    for row in term_rows(capi, torch, synth, args.steps, args.warmup):
        lines.append(dict(config="128x160x16 CS32 K16 term", **row))
    lines.append(dict(config="64x80x16 CS32 sliding", **sliding(capi, torch, synth)))
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
