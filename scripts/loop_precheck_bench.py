#!/usr/bin/env python3
"""The loop detector's candidate loop (LoopDetector::DetectLoop / DetectLocalLoop: MatchGeoCheck on one query keyframe against B
candidates) timed as one call next to the B rounds of single calls it replaces, at 128 x 160, C = 16, K = 512 and 256,
B = 1, 4, 9, 20 (synth.make_loop_candidates).  Two scenes per (K, B): every candidate planted (none pruned), and planted /
unrelated in turn (the unrelated half falls below min_desc_inlier_ratio = 0.3 after the cycle match).

Per row (ms per call; the median of the batches, with the smallest and largest):
  batch_ms          one sage_cycle_match_batch call, pixel_slices = 0; `slices` is the split the library chose
  batch_s1_ms       (B = 1 only) the same with pixel_slices forced to 1
  single_ms         B sage_cycle_match calls on the same inputs
  precheck_ms       one sage_loop_precheck call
  seq3_ms           B rounds of sage_cycle_match -> sage_match_points -> sage_robust_registration, the loop as INTEGRATION.md
                    showed it before (a round stops after the cycle match only when no cycle closed)
  seq3_pruned_ms    the same rounds with the pre-check's ratio test after the cycle match
The single calls are untouched code, so the columns of one run compare the batched path with the path it replaces.  No time
here is a pass criterion.  Prints one JSON line per row, then the table.

    python scripts/loop_precheck_bench.py [--calls 20 --batches 5 --out FILE]
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

H, W, CH = 128, 160, 16
KS, BS = (512, 256), (1, 4, 9, 20)
CYC_THRESH, MULT, MIN_RATIO = 1.0, 2.0, 0.3


def batches_ms(fn, calls, batches, sync):
    for _ in range(max(3, calls // 10)):
        fn()
    sync()
    got = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        got.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(got)), float(min(got)), float(max(got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    ws = capi.Workspace()
    sync = torch.cuda.synchronize
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    slices_of = capi.lib().sage_cycle_match_batch_slices
    slices_of.argtypes = [C.c_void_p]
    recs = []
    for K in KS:
        for B in BS:
            for scene_name in ("none_pruned", "half_pruned"):
                kinds = ["planted"] * B if scene_name == "none_pruned" else [("planted", "unrelated")[b % 2] for b in range(B)]
                sc = synth.make_loop_candidates(1, B, H, W, CH, K, kinds=kinds)
                q = cu(sc["desc_q"])
                cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
                cam = capi.SageCamera(*[float(getattr(sc["cam"], n)) for n in ("fx", "fy", "cx", "cy", "w", "h")])
                i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
                i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
                f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
                raw, cyc, flags, ikp = i64(B, K), i64(B, K), i32(B, K), i32(B, K)
                counts = np.zeros(B, np.int32)
                cand_ptrs = capi._ptr_array([c["desc"] for c in cands]); kp_ptrs = capi._ptr_array([c["kp_loc"] for c in cands])
                d = capi.dptr

                def batch(slices=0):
                    return capi.cycle_match_batch_raw(ws.h, d(q), cand_ptrs, kp_ptrs, B, K, CH, H, W, CYC_THRESH, slices, d(raw), d(cyc), d(flags),
                                                      counts.ctypes.data)

                n1 = C.c_int()

                def single_cm(b):
                    return capi.lib().sage_cycle_match(ws.h, d(q), d(cands[b]["desc"]), d(cands[b]["kp_loc"]), K, CH, H, W, C.c_float(CYC_THRESH),
                                                       d(raw[b]), d(cyc[b]), d(flags[b]), C.byref(n1))

                def singles():
                    for b in range(B):
                        assert single_cm(b) == 0

                # the batch and the singles agree on this scene before anything is timed
                assert batch() == 0
                chosen = int(slices_of(ws.h))
                want = (raw.clone(), cyc.clone(), flags.clone(), counts.copy())
                raw.zero_(); cyc.zero_(); flags.zero_()
                got_n = []
                for b in range(B):
                    assert single_cm(b) == 0
                    got_n.append(n1.value)
                assert torch.equal(raw, want[0]) and torch.equal(cyc, want[1]) and torch.equal(flags, want[2]) and list(want[3]) == got_n

                prm = capi.registration_params(synth.registration_params(1.0))
                results = (capi.SageLoopPrecheckResult * B)()
                arr = (capi.SageLoopCandidate * B)(*[capi.SageLoopCandidate(*[d(c[n]).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")])
                                                     for c in cands])

                def precheck():
                    return capi.loop_precheck_raw(ws.h, d(q), sc["depth_divisor"], C.addressof(arr), B, K, CH, H, W, C.addressof(cam), CYC_THRESH, MULT,
                                                  MIN_RATIO, C.addressof(prm), C.addressof(results), d(raw), d(flags), d(ikp))

                pts0, pts1, homo1, nb, dpts1, kept = f32(K, 3), f32(K, 3), f32(K, 3), f32(K), f32(K), i32(K)
                M, mean = C.c_int(), C.c_float()
                res = capi.SageRegistrationResult()
                inl_dev = i32(K)
                focal = (np.float32(cam.fx) + np.float32(cam.fy)) / np.float32(2)
                seq_out = [None] * B

                def seq3(prune):
                    for b, c in enumerate(cands):
                        assert single_cm(b) == 0
                        seq_out[b] = (n1.value, 0, 0)
                        if n1.value <= 0 or (prune and np.float32(n1.value) / np.float32(K) < np.float32(MIN_RATIO)):
                            continue
                        assert capi.match_points_raw(ws.h, d(flags[b]), d(raw[b]), d(c["kp_dpts0"]), d(c["kp_homo0"]), sc["depth_divisor"], d(c["dpt_map"]),
                                                     C.addressof(cam), K, W, MULT, 1, d(pts0), d(pts1), d(nb), d(homo1), d(dpts1), d(kept),
                                                     C.addressof(M), C.addressof(mean)) == 0
                        p = capi.registration_params(synth.registration_params(float((np.float32(MULT) * np.float32(mean.value)) / focal)))
                        assert capi.robust_registration_raw(ws.h, d(pts0), d(pts1), d(nb), M.value, C.addressof(p), C.addressof(res), None,
                                                            d(inl_dev)) == 0
                        seq_out[b] = (n1.value, M.value, res.n_inliers)

                assert precheck() == 0
                seq3(True)
                registered = [int(r.registered) for r in results]
                assert [(r.n_cycle, r.n_matched, r.reg.n_inliers) for r in results] == seq_out, "the pre-check and the three calls disagree"
                assert registered == [int(k == "planted") for k in kinds], registered

                rec = dict(what="loop_precheck", K=K, B=B, scene=scene_name, H=H, W=W, C=CH, slices=chosen, registered=sum(registered),
                           calls=a.calls, batches=a.batches, device=torch.cuda.get_device_name(0))
                t = {}
                if scene_name == "none_pruned":            # (the cycle match's cost does not depend on what the maps hold)
                    t["batch_ms"] = batches_ms(batch, a.calls, a.batches, sync)
                    t["single_ms"] = batches_ms(singles, a.calls, a.batches, sync)
                    if B == 1:
                        t["batch_s1_ms"] = batches_ms(lambda: batch(1), a.calls, a.batches, sync)
                t["precheck_ms"] = batches_ms(precheck, a.calls, a.batches, sync)
                t["seq3_ms"] = batches_ms(lambda: seq3(False), a.calls, a.batches, sync)
                t["seq3_pruned_ms"] = batches_ms(lambda: seq3(True), a.calls, a.batches, sync)
                for k, v in t.items():
                    rec[k] = v[0]
                    rec[k + "_min_max"] = v[1:]
                if "batch_ms" in t:
                    rec["single_over_batch"] = t["single_ms"][0] / t["batch_ms"][0]
                rec["seq3_over_precheck"] = t["seq3_ms"][0] / t["precheck_ms"][0]
                rec["seq3_pruned_over_precheck"] = t["seq3_pruned_ms"][0] / t["precheck_ms"][0]
                print(json.dumps(rec), flush=True)
                recs.append(rec)

    f = lambda r, k: f"{r[k]:8.3f} [{r[k + '_min_max'][0]:.3f} {r[k + '_min_max'][1]:.3f}]" if k in r else " " * 22
    table = ["", "ms per call: median [min max] of %d batches of %d calls; %s" % (a.batches, a.calls, recs[0]["device"] if recs else ""),
             "cycle match     K   B slices  batch                  B single calls         single/batch  batch, 1 slice"]
    for r in recs:
        if "batch_ms" in r:
            table.append(f"             {r['K']:4d} {r['B']:3d} {r['slices']:6d}  {f(r, 'batch_ms')} {f(r, 'single_ms')} {r['single_over_batch']:8.2f}      {f(r, 'batch_s1_ms')}")
    table.append("pre-check       K   B scene        solves  precheck               3 calls x B            ... with the ratio test  3x/pre  pruned 3x/pre")
    for r in recs:
        table.append(f"             {r['K']:4d} {r['B']:3d} {r['scene']:12s} {r['registered']:6d}  {f(r, 'precheck_ms')} {f(r, 'seq3_ms')} {f(r, 'seq3_pruned_ms')}"
                     f" {r['seq3_over_precheck']:7.2f} {r['seq3_pruned_over_precheck']:7.2f}")
    print("\n".join(table), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in recs) + "\n" + "\n".join(table) + "\n")
    ws.close()


if __name__ == "__main__":
    main()
