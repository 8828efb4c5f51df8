#!/usr/bin/env python3
"""sage_vocabulary_build (DBoW2's hierarchical k-means, all nodes of a level in the same launches) timed next to what an
embedder would write today: the same steps as torch expressions on the same device and inputs, one node at a time -- kmeans++
with cdist / cumsum / searchsorted, Lloyd rounds with cdist + argmin + index_add, one .item() per round for the stop rule.

Configurations (descriptors: synth.make_voc_training_set, kind "planted", documents of 1000 points):
  L3_30k    k = 10, L = 3, C = 16, M = 30 000
  L3_300k   k = 10, L = 3, C = 16, M = 300 000
  L4_300k   k = 10, L = 4, C = 16, M = 300 000
Per configuration: build_ms (median, smallest, largest of the builds; descriptors on the device in, tree and weights out),
rounds (seeding + Lloyd rounds over all levels) and ms per round; torch_ms and its rounds (per node, summed) and nodes; the
ratio torch_ms / build_ms.  The torch expression draws its own random numbers: the two trees differ, the work is of the same
kind and size.  Every configuration runs in a child process under a time limit of its own; the first that fails ends the
run.  Prints one JSON line per configuration.

    python scripts/voc_build_bench.py [--builds 5 --out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"L3_30k": (10, 3, 16, 30), "L3_300k": (10, 3, 16, 300), "L4_300k": (10, 4, 16, 300)}


def torch_build(X, k, L, seed):
    """X [M, C] on the device -> (nodes split, rounds summed over the nodes, leaves)"""
    import torch
    rng = np.random.default_rng(seed)
    nodes = rounds = leaves = 0
    todo = [(torch.arange(X.shape[0], device=X.device), 1)]
    while todo:
        idx, level = todo.pop()
        n = int(idx.numel())
        nodes += 1
        if n <= k:
            leaves += n
            continue
        pts = X[idx]
        centres = [pts[int(rng.random() * n)]]
        min_d = torch.cdist(pts, centres[0][None])[:, 0]
        for r in range(1, k):
            if r > 1:
                d = torch.cdist(pts, centres[-1][None])[:, 0]
                min_d = torch.where((min_d > 0) & (d < min_d), d, min_d)
            run = torch.cumsum(min_d.double(), 0)
            at = torch.searchsorted(run, run[-1:] * rng.random()).clamp_(max=n - 1)
            centres.append(pts[at[0]])
            rounds += 1
        cen = torch.stack(centres)
        assign = torch.cdist(pts, cen).argmin(1)
        rounds += 1
        for _ in range(100):
            sums = torch.zeros_like(cen).index_add_(0, assign, pts)
            cnt = torch.bincount(assign, minlength=k).to(pts.dtype)[:, None]
            cen = torch.where(cnt > 0, sums / cnt.clamp(min=1), cen)
            new = torch.cdist(pts, cen).argmin(1)
            mismatch = int((new != assign).sum().item())
            assign = new
            rounds += 1
            if np.float32(mismatch) / np.float32(n) < 1.0e-3:
                break
        for c in range(k):
            sub = idx[assign == c]
            if level < L and sub.numel() > 1:
                todo.append((sub, level + 1))
            else:
                leaves += 1
    return nodes, rounds, leaves


def child(name, builds):
    import torch
    from sage_slam_amd import capi, synth
    k, L, Cn, n_docs = CONFIGS[name]
    t = synth.make_voc_training_set(k, L, Cn, n_docs, 1000, seed=1, kind="planted")
    desc = torch.from_numpy(t["desc"]).cuda()
    X = desc.t().contiguous()
    ws = capi.Workspace()

    def one():
        b = capi.VocabularyBuild(ws, desc, t["doc_begin"], k=k, L=L, seed=1)
        st = b.stats
        r = (sum(st.seed_rounds) + sum(st.rounds), st.n_nodes, st.n_words, sum(st.launches), sum(st.waits))
        b.close()
        return r

    one()
    ms = []
    for _ in range(builds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = one()
        ms.append(1e3 * (time.perf_counter() - t0))
    torch_build(X, k, L, 1)
    tms = []
    for _ in range(max(1, builds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tinfo = torch_build(X, k, L, 1)
        torch.cuda.synchronize()
        tms.append(1e3 * (time.perf_counter() - t0))
    rounds, n_nodes, n_words, launches, waits = info
    print(json.dumps(dict(config=name, k=k, L=L, C=Cn, M=t["M"], build_ms=round(float(np.median(ms)), 3), build_ms_min=round(min(ms), 3),
                          build_ms_max=round(max(ms), 3), rounds=rounds, ms_per_round=round(float(np.median(ms)) / rounds, 4),
                          n_nodes=n_nodes, n_words=n_words, launches=launches, waits=waits,
                          torch_ms=round(float(np.median(tms)), 3), torch_nodes=tinfo[0], torch_rounds=tinfo[1],
                          torch_over_build=round(float(np.median(tms)) / float(np.median(ms)), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.builds)
        return 0
    lines = []
    for name in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--builds", str(a.builds)], capture_output=True,
                           text=True, timeout=240)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
