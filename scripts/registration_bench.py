#!/usr/bin/env python3
"""Robust registration of keypoint matches (sage_robust_registration; teaser::RobustRegistrationSolver::solve in the
reference's shipped configuration) timed at N = 256 and 512 with 30 % and 70 % outliers (synth.make_registration_problem),
next to the literal torch expression of the solver's steps 1-2 -- the pair tensors, torch.sort of the 2 * pairs endpoints,
cumsum of the running sums, the cost and argmin, one .item() -- through PyTorch-ROCm on the same device and inputs in fp64.

Per configuration:
  reg_ms          one sage_robust_registration call (points and bounds on the device in, result and inlier list on the host
                  out): the device vote, one ticket, the host finish; median over the batches, with the smallest and largest
  reg_ms_by_sort_tile   the same with the sort's LDS tile at 1024, 2048 and 4096 endpoints (SAGE_REG_SORT_TILE; the default is 1024)
  finish_ms       the host finish alone (sage_registration_finish on host copies of the same points at the call's scale)
  torch_vote_ms   the torch expression of steps 1-2 alone (no rotation, no translation)
No time here is a pass criterion.  Prints one JSON line per configuration.

    python scripts/registration_bench.py [--calls 100 --batches 5 --out FILE]
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


def torch_vote(torch, src, dst, nb, ij):
    """steps 1-2 as tensor expressions -> scale (host float)"""
    i, j = ij
    s64, d64, n64 = src.double(), dst.double(), nb.double()
    v1 = (s64[j] - s64[i]).square().sum(1).sqrt()
    v2 = (d64[j] - d64[i]).square().sum(1).sqrt()
    X = v2 / v1
    r = (n64[j] + n64[i]) * (1.0 / v1)
    w = 1.0 / (r * r)
    n = X.numel()
    h = torch.stack([X - r, X + r], 1).reshape(-1)
    _, order = torch.sort(h)
    idx = order // 2
    eps = 1.0 - 2.0 * (order % 2).double()
    ew = eps * w[idx]
    Xs, rs = X[idx], r[idx]
    s_w = torch.cumsum(ew, 0); s_wx = torch.cumsum(ew * Xs, 0); s_r = torch.cumsum(eps * rs, 0)
    s_x = torch.cumsum(eps * Xs, 0); s_xx = torch.cumsum(eps * Xs * Xs, 0); card = torch.cumsum(eps, 0)
    x_hat = s_wx / s_w
    cost = card * x_hat * x_hat + s_xx - 2 * s_x * x_hat + (r.sum() - s_r)
    cost = torch.where(torch.isnan(cost), torch.full_like(cost, float("inf")), cost)
    return float(x_hat[torch.argmin(cost)].item()), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sage_slam_amd import capi, synth
    ws = capi.Workspace()
    sync = torch.cuda.synchronize
    lines = []
    for N, rate in CONFIGS:
        prob = synth.make_registration_problem(N, 1, rate, 0.3, "plain")
        src, dst, nb = (torch.from_numpy(prob[k]).cuda() for k in ("src", "dst", "noise_bounds"))
        p = capi.registration_params(prob["params"])
        res = capi.SageRegistrationResult()
        inl = np.zeros(N, np.int32)
        out = capi.robust_registration(ws, src, dst, nb, p)
        call = lambda: capi.robust_registration_raw(ws.h, capi.dptr(src), capi.dptr(dst), capi.dptr(nb), N, C.addressof(p), C.addressof(res),
                                                    inl.ctypes.data, None)
        assert call() == 0
        reg = batches_ms(call, a.calls, a.batches, sync)
        by_tile = {}
        for tile in (1024, 2048, 4096):   # the sort's LDS tile (SAGE_REG_SORT_TILE, read per call): which one the default should be
            os.environ["SAGE_REG_SORT_TILE"] = str(tile)
            assert call() == 0 and res.scale == out["scale"] and res.n_inliers == out["n_inliers"]
            by_tile[str(tile)] = batches_ms(call, a.calls, 3, sync)[0]
        del os.environ["SAGE_REG_SORT_TILE"]
        hs, hd, hn = prob["src"], prob["dst"], prob["noise_bounds"]
        fin = lambda: capi.registration_finish_raw(hs.ctypes.data, hd.ctypes.data, hn.ctypes.data, N, out["scale"], C.addressof(p),
                                                   C.addressof(res), inl.ctypes.data, None)
        assert fin() == 0
        finish = batches_ms(fin, a.calls, a.batches, lambda: None)
        ij = torch.triu_indices(N, N, 1, device="cuda")
        t_scale, n_pairs = torch_vote(torch, src, dst, nb, ij)
        tv = batches_ms(lambda: torch_vote(torch, src, dst, nb, ij), max(2, a.calls // 10), max(3, a.batches - 2), sync)
        rec = dict(what="registration", N=N, outlier_rate=rate, pairs=n_pairs, endpoints=2 * n_pairs, scale=out["scale"],
                   torch_scale_rel_diff=abs(t_scale - out["scale"]) / out["scale"], n_inliers=out["n_inliers"],
                   n_scale_inlier_pairs=out["n_scale_inlier_pairs"], rotation_iterations=out["rotation_iterations"],
                   reg_ms=reg[0], reg_ms_min_max=reg[1:], reg_ms_by_sort_tile=by_tile, finish_ms=finish[0], finish_ms_min_max=finish[1:], torch_vote_ms=tv[0],
                   torch_vote_ms_min_max=tv[1:], calls=a.calls, batches=a.batches, device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
