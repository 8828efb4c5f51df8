#!/usr/bin/env python3
"""The loop detector's tracking stage (TrackFrame on every survivor of the pre-check: loop_detector.cpp:165, :321) timed as one
batched call next to the B single calls it replaces, in one process, alternating.

Shapes: the headline tracker shape 64 x 80 x 16 (N = 3072 samples) and 128 x 160 x 16 (N = 3072), 4 pyramid levels;
B = 1, 4, 9, 20.  Per (shape, B), ms per call as median [min max] over the batches:
  track_batch_ms    one sage_track_frame_batch (dof 7, photometric + match geometry, NK = 200 keypoints)
  track_single_ms   B sage_track_frame calls on the same problems
  verify_ms         one sage_loop_verify over B planted candidates (K = 256 keypoints: NK = the registration's inliers)
  verify_single_ms  its single-call composition: per candidate sage_track_frame + sage_track_overlap on the keypoint arrays the
                    gather left (the gather itself has no single call: its one launch is left out of this column)
`iters` are the LM iterations of the B problems: a batch runs as many rounds as its longest problem has evaluations, and pays per
round what a single call pays per evaluation.  The script asserts that the batch's poses and iteration counts are the
singles'.  No time here is a pass criterion.  Prints one JSON line per row, then the table.

    python scripts/loop_verify_bench.py [--calls 10 --batches 5 --out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(H=64, W=80), dict(H=128, W=160)]
BS = (1, 4, 9, 20)
N, NK, K, L, FS = 3072, 200, 256, 4, 16
START = dict(rot=(0.004, -0.003, 0.002), trans=(0.004, -0.003, 0.002))
CYC_THRESH, MULT, MG_WEIGHT, DIVISOR = 1.0, 2.0, 3.0, 1.0


def alternate_ms(fns, calls, batches, sync):
    """fns: name -> callable; timed in turn, batch by batch -> name -> (median, min, max) ms per call"""
    for fn in fns.values():
        for _ in range(2):
            fn()
    sync()
    got = {k: [] for k in fns}
    for _ in range(batches):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            got[k].append(1e3 * (time.perf_counter() - t0) / calls)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from oracle import oracle as orc
    from sage_slam_amd import capi, synth
    from tests.test_gpu_tracker import Scene
    orc.build()
    ws = capi.Workspace()
    sync = torch.cuda.synchronize
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cfg = capi.lm_config_default()
    recs = []
    for shape in SHAPES:
        H, W = shape["H"], shape["W"]
        scenes = []
        for seed in (31, 32):
            s = Scene(capi, orc, seed=seed, NK=NK, H=H, W=W, FS=FS, L=L, n_samples=N)
            s.ws.close()
            s.ws = ws
            scenes.append(s)
        n_have = scenes[0].a.homo.shape[0]
        # ---- the pre-check's outputs for 20 planted candidates, once per shape
        sc = synth.make_loop_candidates(1, max(BS), H, W, 16, K, kinds=["planted"] * max(BS), grid=2)
        cam = sc["cam"]
        ccam = capi.SageCamera(*[float(getattr(cam, n)) for n in ("fx", "fy", "cx", "cy", "w", "h")])
        cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
        q0 = scenes[0]
        vy, vx = np.nonzero(q0.w.mask > 0.5)
        vhomo = cu(np.stack([(vx - cam.cx) / cam.fx, (vy - cam.cy) / cam.fy, np.ones(vx.size)], 1).astype(np.float32))
        vd = cu((q0.a.bias + q0.a.basis @ q0.a.code_true)[vy * W + vx].astype(np.float32))
        query = capi.SageLoopVerifyQuery()
        query.N = n_have; query.FS = FS
        query.homo_dev = q0.dev["homo"].data_ptr(); query.unscaled_dpts0_dev = q0.dev["unscaled"].data_ptr()
        query.feat0s_dev = q0.dev["f0s"].data_ptr(); query.weights_dev = q0.dev["wts"].data_ptr()
        query.pyr = capi.make_pyramid(cam, L); query.eps = q0.w.eps
        query.M = int(vx.size); query.valid_homo_dev = vhomo.data_ptr(); query.valid_dpts0_dev = vd.data_ptr()
        query.mask_dev = q0.dev["mask"].data_ptr()
        for B in BS:
            # ---- sage_track_frame_batch next to B sage_track_frame
            probs = [scenes[b % 2].problem(7, True, True) for b in range(B)]
            starts = [(scenes[b % 2].start_pose(tuple((1 + 0.25 * (b // 2)) * np.array(START["rot"])),
                                                tuple((1 + 0.25 * (b // 2)) * np.array(START["trans"]))),
                       float(scenes[b % 2].s_true) * 0.96) for b in range(B)]

            def singles():
                return [capi.track_frame(cfg, 7, p, pose, s) for p, (pose, s) in zip(probs, starts)]

            def batch():
                return capi.track_frame_batch(cfg, 7, probs, [p for p, _ in starts], [s for _, s in starts])

            one = singles()
            got = batch()
            assert got[0] == 0 and all(r[0] == 0 for r in one)
            assert all(np.array_equal(got[1][b], one[b][1]) and int(got[4][b]) == one[b][4] for b in range(B)), "batch != singles"
            iters = [r[4] for r in one]
            t = alternate_ms(dict(track_batch_ms=batch, track_single_ms=singles), a.calls, a.batches, sync)
            # ---- sage_loop_verify next to its composition
            arr = (capi.SageLoopCandidate * B)(*[capi.SageLoopCandidate(*[capi.dptr(c[n]).value for n in ("desc", "dpt_map", "kp_loc",
                                                                                                     "kp_dpts0", "kp_homo0")])
                                                 for c in cands[:B]])
            prm = capi.registration_params(synth.registration_params(1.0))
            pre = (capi.SageLoopPrecheckResult * B)()
            raw = torch.zeros(B, K, dtype=torch.int64, device="cuda")
            flags = torch.zeros(B, K, dtype=torch.int32, device="cuda")
            ikp = torch.zeros(B, K, dtype=torch.int32, device="cuda")
            desc_q = cu(sc["desc_q"])
            rc = capi.loop_precheck_raw(ws.h, capi.dptr(desc_q), DIVISOR, C.addressof(arr), B, K, 16, H, W, C.addressof(ccam), CYC_THRESH,
                                        MULT, 0.3, C.addressof(prm), C.addressof(pre), capi.dptr(raw), capi.dptr(flags), capi.dptr(ikp))
            assert rc == 0
            n_surv = sum(1 for b in range(B) if pre[b].registered == 1 and pre[b].reg.n_inliers > 3)
            vc = [dict(feat1=scenes[b % 2].dev["feat1"], grad1=scenes[b % 2].dev["grad1"], mask1=scenes[b % 2].dev["mask"],
                       kp_loss_param=q0.mg_loss_param) for b in range(B)]
            res, gathered = capi.loop_verify(ws, cfg, query, DIVISOR, cands[:B], vc, pre, raw, ikp, MG_WEIGHT)
            comp = []
            for b in range(B):
                if not res[b].tracked:
                    continue
                p = capi.SageTrackProblem()
                p.ws = ws.h; p.use_photo = 1; p.use_keypoints = 1
                p.mask1_dev = vc[b]["mask1"].data_ptr(); p.feat1_dev = vc[b]["feat1"].data_ptr(); p.grad1_dev = vc[b]["grad1"].data_ptr()
                p.dpts0_dev = query.unscaled_dpts0_dev; p.homo_dev = query.homo_dev; p.feat0s_dev = query.feat0s_dev
                p.weights_dev = query.weights_dev; p.pyr = query.pyr; p.eps = query.eps; p.N = query.N; p.FS = FS
                p.NK = pre[b].reg.n_inliers
                base = gathered.data_ptr() + b * 8 * K * 4
                p.kp_homo0_dev = base; p.kp_dpts0_dev = base + 3 * K * 4; p.kp_matched_homo1_dev = base + 4 * K * 4
                p.kp_matched_dpts1_dev = base + 7 * K * 4
                p.kp_loss_param = vc[b]["kp_loss_param"]
                p.kp_weight = float(np.float32(pre[b].desc_match_inlier_ratio) * np.float32(MG_WEIGHT))
                pose0 = np.concatenate([np.array(pre[b].reg.R[:]), np.array(pre[b].reg.t[:])]).astype(np.float32)
                comp.append((p, pose0, float(np.float32(pre[b].reg.scale))))

            def verify():
                return capi.loop_verify(ws, cfg, query, DIVISOR, cands[:B], vc, pre, raw, ikp, MG_WEIGHT)

            def verify_single():
                for p, pose0, s0 in comp:
                    rc, ph, sh, eh, it, _ = capi.track_frame(cfg, 7, p, pose0, s0)
                    capi.track_overlap(ws, ph[:9], ph[9:], vd, vhomo, cam, q0.dev["mask"], query.eps,
                                       depth_scale=float(np.float32(sh) / np.float32(DIVISOR)))

            t.update(alternate_ms(dict(verify_ms=verify, verify_single_ms=verify_single), a.calls, a.batches, sync))
            rec = dict(shape=f"{H}x{W}x{FS}", N=n_have, B=B, iters=iters, verify_survivors=n_surv,
                       verify_iters=[int(res[b].iters) for b in range(B) if res[b].tracked],
                       **{k: [round(x, 4) for x in v] for k, v in t.items()})
            rec["track_speedup"] = round(t["track_single_ms"][0] / t["track_batch_ms"][0], 2)
            rec["verify_speedup"] = round(t["verify_single_ms"][0] / t["verify_ms"][0], 2)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    lines = ["shape       B  track_batch_ms [min max]    track_single_ms [min max]   x     verify_ms [min max]         "
             "verify_single_ms [min max]  x     iterations (max)"]
    f3 = lambda v: f"{v[0]:7.3f} [{v[1]:7.3f} {v[2]:7.3f}]"
    for r in recs:
        lines.append(f"{r['shape']:11s} {r['B']:2d}  {f3(r['track_batch_ms'])}   {f3(r['track_single_ms'])}  {r['track_speedup']:5.2f}  "
                     f"{f3(r['verify_ms'])}   {f3(r['verify_single_ms'])}  {r['verify_speedup']:5.2f}  {max(r['iters'])}")
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")
            fh.write("\n" + table + "\n")


if __name__ == "__main__":
    main()
