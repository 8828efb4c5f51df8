#!/usr/bin/env python3
"""B robust registrations in one call (sage_robust_registration_batch: the scale votes of all problems in one sort) timed next
to the B unchanged sage_robust_registration calls they replace, on the same inputs in the same process, the two alternating
batch by batch.  Problems from synth.make_registration_problem (seed b for problem b): N = 256 and 512 at 30 % and 70 %
outliers, B = 1, 4, 9, 20, and one batch of mixed sizes (N = 512, 384, 256, 200, 128, 92, 91, 64, 33, at 30 %).

Per row (ms per call; the median of the batches, with the smallest and largest):
  batch_ms        one sage_robust_registration_batch call (points and bounds on the device in, results and inlier rows on the
                  host out): the device votes, one ticket, the B host finishes
  singles_ms      B sage_robust_registration calls
  ratio           singles_ms / batch_ms
  finish_ms       the B host finishes alone (sage_registration_finish on host copies of the points at the calls' scales);
                  finish_share = finish_ms / batch_ms
  launches        what the batch spent (sage_robust_registration_batch_launches); the B single calls spend B (launches - 1)
                  (B = 1 takes the single call's path: the same launches)
  batch_ms_by_sort_tile   (B = 20 and the mixed batch) the batch with the sort's LDS tile at 1024, 2048 and 4096 endpoints
                  (SAGE_REG_SORT_TILE; the default is 1024), three batches each
Before anything is timed the rows of the batch are compared with the single calls' results for equality.  No time here is a
pass criterion.  Prints one JSON line per row, then the table.

    python scripts/registration_batch_bench.py [--calls 50 --batches 5 --out FILE]
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

CONFIGS = [(256, 0.3), (256, 0.7), (512, 0.3), (512, 0.7)]
BS = (1, 4, 9, 20)
MIXED = (512, 384, 256, 200, 128, 92, 91, 64, 33)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    ws = capi.Workspace()
    sync = torch.cuda.synchronize
    d = capi.dptr
    rows = [("N=%d" % N, rate, [N] * B) for N, rate in CONFIGS for B in BS] + [("mixed", 0.3, list(MIXED))]
    recs = []
    for name, rate, Ns in rows:
        B = len(Ns)
        host = [synth.make_registration_problem(N, b, rate, 0.3, "plain") for b, N in enumerate(Ns)]
        dev = [{k: torch.from_numpy(q[k]).cuda() for k in ("src", "dst", "noise_bounds")} for q in host]
        prm = [capi.registration_params(q["params"]) for q in host]
        stride = max(Ns)
        probs = (capi.SageRegistrationProblem * B)(*[capi.SageRegistrationProblem(d(t["src"]).value, d(t["dst"]).value, d(t["noise_bounds"]).value,
                                                                                  N, q["params"]["noise_bound"], None)
                                                     for t, q, N in zip(dev, host, Ns)])
        res_b = (capi.SageRegistrationResult * B)()
        res_s = (capi.SageRegistrationResult * B)()
        inl_b = np.zeros((B, stride), np.int32); inl_s = np.zeros((B, stride), np.int32)
        shared = capi.registration_params(host[0]["params"])

        def batch():
            assert capi.robust_registration_batch_raw(ws.h, C.addressof(probs), B, C.addressof(shared), C.addressof(res_b), inl_b.ctypes.data,
                                                      stride) == 0

        def singles():
            for b in range(B):
                assert capi.robust_registration_raw(ws.h, d(dev[b]["src"]), d(dev[b]["dst"]), d(dev[b]["noise_bounds"]), Ns[b],
                                                    C.addressof(prm[b]), C.addressof(res_s[b]), inl_s[b].ctypes.data, None) == 0

        res_f = capi.SageRegistrationResult()
        inl_f = np.zeros(stride, np.int32)

        def finishes():
            for b in range(B):
                q = host[b]
                assert capi.registration_finish_raw(q["src"].ctypes.data, q["dst"].ctypes.data, q["noise_bounds"].ctypes.data, Ns[b],
                                                    res_s[b].scale, C.addressof(prm[b]), C.addressof(res_f), inl_f.ctypes.data, None) == 0

        batch(); singles()
        assert bytes(res_b) == bytes(res_s) and inl_b.tobytes() == inl_s.tobytes(), "the batch and the single calls disagree"
        assert all(r.valid == 1 for r in res_b)
        launches = capi.robust_registration_batch_launches(ws)
        assert launches == capi.robust_registration_batch_plan(Ns)["launches"]
        t_batch, t_singles = alternating_ms([batch, singles], a.calls, a.batches, sync)
        t_finish = alternating_ms([finishes], a.calls, a.batches, lambda: None)[0]
        by_tile = {}
        if B == BS[-1] or name == "mixed":   # the sort's LDS tile (SAGE_REG_SORT_TILE, read per call): the same bytes, another time
            for tile in (1024, 2048, 4096):
                os.environ["SAGE_REG_SORT_TILE"] = str(tile)
                batch()
                assert bytes(res_b) == bytes(res_s) and inl_b.tobytes() == inl_s.tobytes(), "another sort tile, other bytes"
                by_tile[str(tile)] = alternating_ms([batch], a.calls, 3, sync)[0][0]
            del os.environ["SAGE_REG_SORT_TILE"]
        rec = dict(what="registration_batch", problems=name, outlier_rate=rate, B=B, N=Ns if name == "mixed" else Ns[0], launches=launches,
                   batch_ms=t_batch[0], batch_ms_min_max=t_batch[1:], singles_ms=t_singles[0], singles_ms_min_max=t_singles[1:],
                   ratio=t_singles[0] / t_batch[0], finish_ms=t_finish[0], finish_ms_min_max=t_finish[1:],
                   finish_share=t_finish[0] / t_batch[0], batch_ms_by_sort_tile=by_tile, calls=a.calls, batches=a.batches, device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    f = lambda r, k: f"{r[k]:8.3f} [{r[k + '_min_max'][0]:.3f} {r[k + '_min_max'][1]:.3f}]"
    table = ["", "ms per call: median [min max] of %d batches of %d calls, the batch and the single calls alternating; %s"
             % (a.batches, a.calls, recs[0]["device"] if recs else ""),
             "problems outliers   B launches  batch                  B single calls         singles/batch  B finishes (host)      share of the batch"]
    for r in recs:
        table.append(f"{r['problems']:8s} {r['outlier_rate']:8.1f} {r['B']:3d} {r['launches']:8d}  {f(r, 'batch_ms')} {f(r, 'singles_ms')} {r['ratio']:9.2f}"
                     f"      {f(r, 'finish_ms')} {r['finish_share']:8.2f}"
                     + ("      tiles 1024 / 2048 / 4096: " + " / ".join(f"{r['batch_ms_by_sort_tile'][k]:.3f}" for k in ("1024", "2048", "4096"))
                        if r["batch_ms_by_sort_tile"] else ""))
    print("\n".join(table), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(r) for r in recs) + "\n" + "\n".join(table) + "\n")
    ws.close()


if __name__ == "__main__":
    main()
