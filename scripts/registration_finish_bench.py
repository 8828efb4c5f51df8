#!/usr/bin/env python3
"""The finish of a batch of registrations on the host (SAGE_REG_FINISH_HOST: sage_registration_finish on the calling thread,
serially, in row order) and on the device (SAGE_REG_FINISH_DEVICE: reg_finish_kernel, one workgroup per problem behind the
vote) timed next to each other: sage_robust_registration_batch on two workspaces of one process, one per mode, the two
alternating batch by batch on the same inputs.  Problems from synth.make_registration_problem (seed b for problem b, 30 %
outliers): N = 256 and 512 at B = 1, 4, 9, 20, and the mixed batch of scripts/registration_batch_bench.py (N = 512, 384,
256, 200, 128, 92, 91, 64, 33).  Then sage_loop_precheck at 128 x 160, C = 16, K = 512 and 256, B = 20, every candidate
planted (scripts/loop_precheck_bench.py's scene), in both modes.

Per row (ms per call; the median of the batches, with the smallest and largest):
  host_ms         the call in HOST mode                      device_ms      the call in DEVICE mode
  ratio           host_ms / device_ms                        launches       what each mode spent (host / device)
  finish_host_ms  the B host finishes alone (sage_registration_finish on host copies of the points at the calls' scales)
  finish_dev_ms   the device finish alone (sage_registration_finish_batch at the same scales: one launch, the ticket, one wait)
  outside         yes: the [min max] ranges of host_ms and device_ms do not overlap (the difference lies outside the spread)
Before anything is timed the two modes' results are compared: counts, lists and iterations equal, R and t to 1e-9.  No time
here is a pass criterion.  Prints one JSON line per row, then the table.

    python scripts/registration_finish_bench.py [--calls 50 --batches 5 --out FILE]
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

NS, BS = (256, 512), (1, 4, 9, 20)
MIXED = (512, 384, 256, 200, 128, 92, 91, 64, 33)
RATE = 0.3
H, W, CH = 128, 160, 16
CYC_THRESH, MULT, MIN_RATIO = 1.0, 2.0, 0.3


def alternating_ms(fns, calls, batches, sync):
    """-> per function (median, min, max) ms per call; in every batch the functions run one after the other"""
    for fn in fns:
        for _ in range(max(3, calls // 10)):
            fn()
    sync()
    got = [[] for _ in fns]
    for _ in range(batches):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            got[i].append(1e3 * (time.perf_counter() - t0) / calls)
    return [(float(np.median(g)), float(min(g)), float(max(g))) for g in got]


def outside(a, b):
    return a[1] > b[2] or b[1] > a[2]


def same_result(h, d):
    for k in ("valid", "n_inliers", "n_pairs", "n_degenerate_pairs", "n_scale_inlier_pairs", "rotation_iterations", "n_rotation_inliers"):
        assert getattr(h, k) == getattr(d, k), k
    assert h.scale == d.scale and h.scale_cost == d.scale_cost
    assert np.allclose(list(h.R), list(d.R), rtol=0, atol=1e-9) and np.allclose(list(h.t), list(d.t), rtol=0, atol=1e-9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    ws_h, ws_d = capi.Workspace(), capi.Workspace()
    ws_d.set_registration_finish(capi.SAGE_REG_FINISH_DEVICE)
    sync = torch.cuda.synchronize
    d = capi.dptr
    device = torch.cuda.get_device_name(0)
    rows = [("N=%d" % N, [N] * B) for N in NS for B in BS] + [("mixed", list(MIXED))]
    recs = []
    for name, Ns in rows:
        B = len(Ns)
        host = [synth.make_registration_problem(N, b, RATE, 0.3, "plain") for b, N in enumerate(Ns)]
        dev = [{k: torch.from_numpy(q[k]).cuda() for k in ("src", "dst", "noise_bounds")} for q in host]
        prm = [capi.registration_params(q["params"]) for q in host]
        stride = max(Ns)
        probs = (capi.SageRegistrationProblem * B)(*[capi.SageRegistrationProblem(d(t["src"]).value, d(t["dst"]).value, d(t["noise_bounds"]).value,
                                                                                  N, q["params"]["noise_bound"], None)
                                                     for t, q, N in zip(dev, host, Ns)])
        res = {m: (capi.SageRegistrationResult * B)() for m in "hdf"}
        inl = {m: np.zeros((B, stride), np.int32) for m in "hdf"}
        shared = capi.registration_params(host[0]["params"])

        def call(ws, m):
            assert capi.robust_registration_batch_raw(ws.h, C.addressof(probs), B, C.addressof(shared), C.addressof(res[m]), inl[m].ctypes.data,
                                                      stride) == 0

        call(ws_h, "h"); launches_h = capi.robust_registration_batch_launches(ws_h)
        call(ws_d, "d"); launches_d = capi.robust_registration_batch_launches(ws_d)
        assert launches_d == capi.registration_finish_plan(Ns)["launches"] == launches_h + 1
        for b in range(B):
            same_result(res["h"][b], res["d"][b])
        assert inl["h"].tobytes() == inl["d"].tobytes(), "the two modes' inlier lists disagree"
        scales = np.array([r.scale for r in res["h"]])
        res_f = capi.SageRegistrationResult()
        inl_f = np.zeros(stride, np.int32)

        def finish_host():
            for b in range(B):
                q = host[b]
                assert capi.registration_finish_raw(q["src"].ctypes.data, q["dst"].ctypes.data, q["noise_bounds"].ctypes.data, Ns[b],
                                                    scales[b], C.addressof(prm[b]), C.addressof(res_f), inl_f.ctypes.data, None) == 0

        def finish_dev():
            assert capi.registration_finish_batch_raw(ws_d.h, C.addressof(probs), B, scales.ctypes.data, C.addressof(shared),
                                                      C.addressof(res["f"]), inl["f"].ctypes.data, stride, None) == 0

        finish_dev()
        assert inl["f"].tobytes() == inl["d"].tobytes()
        t_h, t_d = alternating_ms([lambda: call(ws_h, "h"), lambda: call(ws_d, "d")], a.calls, a.batches, sync)
        t_fh, t_fd = alternating_ms([finish_host, finish_dev], a.calls, a.batches, sync)
        rec = dict(what="registration_finish", problems=name, outlier_rate=RATE, B=B, N=Ns if name == "mixed" else Ns[0],
                   launches_host=launches_h, launches_device=launches_d, host_ms=t_h[0], host_ms_min_max=t_h[1:], device_ms=t_d[0],
                   device_ms_min_max=t_d[1:], ratio=t_h[0] / t_d[0], outside_spread=outside(t_h, t_d), finish_host_ms=t_fh[0],
                   finish_host_ms_min_max=t_fh[1:], finish_dev_ms=t_fd[0], finish_dev_ms_min_max=t_fd[1:], calls=a.calls, batches=a.batches,
                   device=device)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    pre = []
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for K in (512, 256):
        B = 20
        sc = synth.make_loop_candidates(1, B, H, W, CH, K, kinds=["planted"] * B)
        q = cu(sc["desc_q"])
        cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
        cam = capi.SageCamera(*[float(getattr(sc["cam"], n)) for n in ("fx", "fy", "cx", "cy", "w", "h")])
        raw = torch.zeros(B, K, dtype=torch.int64, device="cuda")
        flags = torch.zeros(B, K, dtype=torch.int32, device="cuda")
        ikp = {m: torch.zeros(B, K, dtype=torch.int32, device="cuda") for m in "hd"}
        prm = capi.registration_params(synth.registration_params(1.0))
        results = {m: (capi.SageLoopPrecheckResult * B)() for m in "hd"}
        arr = (capi.SageLoopCandidate * B)(*[capi.SageLoopCandidate(*[d(c[n]).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")])
                                             for c in cands])

        def precheck(ws, m):
            assert capi.loop_precheck_raw(ws.h, d(q), sc["depth_divisor"], C.addressof(arr), B, K, CH, H, W, C.addressof(cam), CYC_THRESH, MULT,
                                          MIN_RATIO, C.addressof(prm), C.addressof(results[m]), d(raw), d(flags), d(ikp[m])) == 0

        precheck(ws_h, "h"); precheck(ws_d, "d")
        for b in range(B):
            assert results["h"][b].registered == results["d"][b].registered == 1
            same_result(results["h"][b].reg, results["d"][b].reg)
            n = results["h"][b].reg.n_inliers
            assert torch.equal(ikp["h"][b, :n], ikp["d"][b, :n])
        t_h, t_d = alternating_ms([lambda: precheck(ws_h, "h"), lambda: precheck(ws_d, "d")], max(a.calls // 2, 5), a.batches, sync)
        rec = dict(what="loop_precheck_finish", K=K, B=B, host_ms=t_h[0], host_ms_min_max=t_h[1:], device_ms=t_d[0], device_ms_min_max=t_d[1:],
                   ratio=t_h[0] / t_d[0], outside_spread=outside(t_h, t_d), calls=max(a.calls // 2, 5), batches=a.batches, device=device)
        print(json.dumps(rec), flush=True)
        pre.append(rec)

    f = lambda r, k: f"{r[k]:8.3f} [{r[k + '_min_max'][0]:.3f} {r[k + '_min_max'][1]:.3f}]"
    table = ["", "sage_robust_registration_batch, ms per call: median [min max] of %d batches of %d calls, the two modes alternating; %s"
             % (a.batches, a.calls, device),
             "problems   B launches  HOST mode              DEVICE mode            host/device outside   B finishes (host)      device finish alone"]
    for r in recs:
        table.append(f"{r['problems']:8s} {r['B']:3d} {r['launches_host']:4d}/{r['launches_device']:<4d} {f(r, 'host_ms')} {f(r, 'device_ms')} {r['ratio']:9.2f}"
                     f"   {'yes' if r['outside_spread'] else 'no ':3s}     {f(r, 'finish_host_ms')} {f(r, 'finish_dev_ms')}")
    table += ["", "sage_loop_precheck at %d x %d, C = %d, every candidate planted, ms per call" % (H, W, CH),
              "  K   B  HOST mode              DEVICE mode            host/device outside"]
    for r in pre:
        table.append(f"{r['K']:4d} {r['B']:3d} {f(r, 'host_ms')} {f(r, 'device_ms')} {r['ratio']:9.2f}   {'yes' if r['outside_spread'] else 'no'}")
    print("\n".join(table), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in recs + pre) + "\n" + "\n".join(table) + "\n")
    ws_h.close(); ws_d.close()


if __name__ == "__main__":
    main()
