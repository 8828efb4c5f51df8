#!/usr/bin/env python3
"""The loop detector's bag of words (sage_bow_transform; TemplatedTensorVocabulary::transform of LoopDetector::AddKeyframe)
timed next to the embedder's alternative today: the literal torch expression of tensor_vocabulary.cpp:131-245 (recursive
index / broadcast subtraction / sum / argmin per inner node, nonzero and .item() per child) through PyTorch-ROCm on the same
device and inputs.

Configurations (descriptors: synth.make_bow_problem, kind "nodes", under the eroded mask):
  shipped  128x160   tests/golden/bow_voc.yml.gz (k = 10, L = 3, C = 16: the whole tree is staged in LDS), M = 16 128
  L4       128x160   synth.make_vocabulary(10, 4, 16): voc_builder's default shape, 11 111 nodes -- the last level no longer
                     fits the LDS budget and is read from global memory
  shipped  256x320   M = 72 960
Per configuration:
  bow_ms            one sage_bow_transform call (descriptor map + valid locations in, vector and statistics out): the walk,
                    the compaction, one ticket; median over the batches, with the smallest and largest batch
  bow_nolds_ms      the same with the LDS staging budget at 0 (SAGE_BOW_LDS_BUDGET=0 when the vocabulary is created): every
                    level read from global memory; the batches of the two alternate
  torch_ms          the literal torch expression; its sequences (inner nodes visited) and .item() calls are counted
Every configuration runs in a child process under a time limit of its own; the first that fails ends the run.  Prints one
JSON line per configuration.

    python scripts/bow_bench.py [--calls 200 --batches 5 --out FILE]
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

CONFIGS = {"shipped_128x160": ("shipped", 128, 160), "L4_128x160": ("L4", 128, 160), "shipped_256x320": ("shipped", 256, 320)}


def batches_ms(fns, calls, batches, sync):
    """the functions' batches alternate -> per function (median, min, max) of ms per call over the batches"""
    for fn in fns:
        for _ in range(max(3, calls // 10)):
            fn()
    sync()
    got = [[] for _ in fns]
    for _ in range(batches):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            got[k].append(1e3 * (time.perf_counter() - t0) / calls)
    return [(float(np.median(g)), float(min(g)), float(max(g))) for g in got]


def child(name, calls, batches):
    import ctypes as C
    import torch
    from sage_slam_amd import capi, synth, vocabulary
    which, H, W = CONFIGS[name]
    v = vocabulary.load_opencv_yaml(os.path.join(ROOT, "tests", "golden", "bow_voc.yml.gz")) if which == "shipped" \
        else synth.make_vocabulary(10, 4, 16, seed=0)
    prob = synth.make_bow_problem(H, W, v["C"], 0, "nodes", v)
    dv = lambda x, t=np.float32: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()
    desc, loc = dv(prob["desc"]), dv(prob["loc1d"], np.int64)
    M, P = prob["M"], prob["P"]
    sync = torch.cuda.synchronize
    voc = capi.Vocabulary(v)
    os.environ["SAGE_BOW_LDS_BUDGET"] = "0"
    voc0 = capi.Vocabulary(v)
    del os.environ["SAGE_BOW_LDS_BUDGET"]
    assert voc0.staged_nodes == 0
    ws = capi.Workspace()
    ids, vals, st = capi.bow_transform(ws, voc, desc, loc)
    ids0, vals0, _ = capi.bow_transform(ws, voc0, desc, loc)
    assert np.array_equal(ids, ids0) and vals.tobytes() == vals0.tobytes()
    # --- the engine: arguments built once, the call itself timed
    cap = min(M, voc.num_words)
    hid = np.empty(cap, np.int32); hval = np.empty(cap, np.float64)
    out = capi.SageBowStats()
    args = lambda vh: (ws.h, vh, capi.dptr(desc), capi.dptr(loc), M, P, hid.ctypes.data, hval.ctypes.data, cap, None, C.addressof(out))
    a1, a0 = args(voc.h), args(voc0.h)
    (bow, nolds) = batches_ms([lambda: capi.bow_transform_raw(*a1), lambda: capi.bow_transform_raw(*a0)], calls, batches, sync)

    # --- the embedder's alternative: tensor_vocabulary.cpp:131-245 on the device
    kids = [[] for _ in range(v["n_nodes"])]
    for i in range(1, v["n_nodes"]):
        kids[int(v["parent"][i])].append(i)
    child_idx = [torch.tensor(k, dtype=torch.long, device="cuda") if k else None for k in kids]
    node_desc = dv(v["descriptors"].T)                                         # C x N
    count = dict(seq=0, item=0)

    def torch_way():
        features = desc.reshape(v["C"], -1)[:, loc]                            # AddKeyframe's gather
        bow = {}
        count["seq"] = count["item"] = 0

        def descend(sub, idx, at):
            ch = child_idx[at]
            cd = node_desc[:, ch]
            Cn, S, K = sub.size(0), sub.size(1), cd.size(1)
            dist = torch.sum(torch.square(sub.reshape(Cn, S, 1) - cd.reshape(Cn, 1, K)), 0, False)
            cl = torch.argmin(dist, 1, False).to(torch.long)
            count["seq"] += 1
            for i in range(K):
                within = torch.nonzero(cl == i).reshape(-1)
                if within.size(0) >= 1:
                    count["item"] += 1
                    subset(within if idx is None else idx[within], int(ch[i].item()))

        def subset(idx, at):
            if not kids[at]:
                w = float(v["weight"][at])
                if w > 0:
                    word = int(v["word_id"][at])
                    bow[word] = bow.get(word, 0.0) + w * features.size(1)
                return
            descend(features[:, idx], idx, at)

        descend(features, None, 0)
        return bow

    words = sorted(torch_way())
    (torch_t,) = batches_ms([torch_way], max(calls // 100, 2), min(batches, 3), sync)
    ws.close()
    return dict(what="bow", config=name, vocabulary=which, size=f"{H}x{W}", M=M, nodes=voc.num_nodes, words=voc.num_words,
                staged_nodes=voc.staged_nodes, n_words_hit=int(st.n_leaves_hit), n_inner_nodes_hit=int(st.n_inner_nodes_hit),
                bow_ms=bow[0], bow_ms_min_max=bow[1:], bow_nolds_ms=nolds[0], bow_nolds_ms_min_max=nolds[1:],
                torch_ms=torch_t[0], torch_ms_min_max=torch_t[1:], torch_sequences=count["seq"], torch_items=count["item"],
                same_words_as_torch=bool(words == ids.tolist()), calls=calls, batches=batches,
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=150, help="seconds per configuration (child process)")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(child(args.child, args.calls, args.batches)))
        return 0
    lines = []
    for name in args.configs.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--batches", str(args.batches),
                                "--child", name], capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"bow_bench: {name} ran into its {args.timeout} s limit; stopping", file=sys.stderr)
            return 124
        got = [l[7:] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"bow_bench: {name} failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            return r.returncode or 1
        print(got[0], flush=True)
        lines.append(got[0])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
