"""numpy restatement of sage_vocabulary_build, written from the description in include/sage_ba.h ("training the
vocabulary"; test infrastructure: the library shares no code with it).  It runs DBoW2's own recursion -- one node at a
time, depth-first in child order --, so the node numbering comes out of the order of creation, not out of a renumbering:

  draw        the counter-based generator: draw j of the node at a path
  seed_node   kmeans++ seeding of one node: distances in fp64 (the L2 norm, not its square), the running sums sequential
              in fp64 (np.cumsum), the cut from the draw with the redraw while it is 0, the first index that reaches it
  kmeans_node seeding, then Lloyd rounds: fp64 distances, the first smallest wins, the exactly rounded mean (math.fsum, one
              division in fp64, one rounding to fp32), an emptied cluster keeps its centre, the stop rule in float, the cap
  build       the tree, the words (leaves in ascending node id), Ni through tests/bow_ref.py's fp64 walk, the weights

and reports what the GPU test's equality rests on:
  min_margin   the smallest relative margin any point met in any Lloyd round: (d_second - d_best) / d_second over the
               squared distances
  min_mean_gap per mean computed, how far the fp64 mean is from the nearest fp32 rounding boundary, in units of the error
               a sequential fp64 sum of the n values can have, (n + 2) 2^-53 mean|x|: above 1, every summation order rounds
               to the same fp32 centre; infinite where the fp64 sum is exact in every order
  min_cut_gap  per seeding pick the relative distance |S - cut| / cut between the cut and the nearer of the two running sums
               around it (the one that reaches it, the one before)
"""
import math

import numpy as np

from tests import bow_ref

_MASK = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15
TF_IDF, TF, IDF, BINARY = range(4)


def _mix(z):
    z &= _MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def draw(seed, path, j):
    h = _mix(seed + _G)
    for c in path:
        h = _mix((h ^ (int(c) & _MASK)) + _G)
    return _mix(h + (j + 1) * _G)


def unit(d):
    return float(d >> 11) * 2.0 ** -53


def _dist2(X, c):
    """fp64 squared distances of the rows of X (float32) to c (float32)"""
    e = X.astype(np.float64) - c.astype(np.float64)[None, :]
    return (e * e).sum(axis=1)


def seed_node(X, k, seed, path, report):
    """X [n, C] float32, n > k -> the positions picked (1..k of them)"""
    n = X.shape[0]
    picks = [min(n - 1, int(unit(draw(seed, path, 0)) * float(n)))]
    min_d = np.sqrt(_dist2(X, X[picks[0]]))
    for r in range(1, k):
        if r > 1:
            d = np.sqrt(_dist2(X, X[picks[-1]]))
            min_d = np.where((min_d > 0) & (d < min_d), d, min_d)
        running = np.cumsum(min_d)                       # sequential
        dist_sum = float(running[-1])
        if not dist_sum > 0:
            break
        cut = dist_sum
        for a in range(64):
            c = unit(draw(seed, path, r + a * k)) * dist_sum
            if c != 0.0:
                cut = c
                break
        at = int(np.searchsorted(running, cut, side="left"))   # the first running sum >= cut
        if at >= n:
            at = n - 1
        before = float(running[at - 1]) if at > 0 else 0.0
        report["min_cut_gap"] = min(report["min_cut_gap"], min(abs(float(running[at]) - cut), abs(cut - before)) / cut)
        report["picks"] += 1
        picks.append(at)
    report["node_picks"].append((tuple(path), tuple(picks)))
    return picks


def _assign(X, centres, report):
    D = np.stack([_dist2(X, c) for c in centres], axis=1)
    best = np.argmin(D, axis=1)                              # the first smallest
    if len(centres) > 1:
        order = np.argsort(D, axis=1, kind="stable")
        rows = np.arange(X.shape[0])
        d0, d1 = D[rows, order[:, 0]], D[rows, order[:, 1]]
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.where(d1 > 0, (d1 - d0) / d1, 0.0)
        # identical centres (duplicates picked apart by the seeding cannot happen: min_d > 0; equal means can) tie exactly in
        # every arithmetic: the first wins there too
        m = np.where((centres[order[:, 0]] == centres[order[:, 1]]).all(axis=1), np.inf, m)
        report["min_margin"] = min(report["min_margin"], float(m.min()))
    return best


def mean_f32(X, report=None):
    """the exactly rounded mean of the rows of X (float32): fsum, one division, one rounding to fp32"""
    n = X.shape[0]
    m64 = np.array([math.fsum(X[:, ch].astype(np.float64).tolist()) / float(n) for ch in range(X.shape[1])], np.float64)
    m32 = m64.astype(np.float32)
    if report is not None:
        a32 = np.abs(m32)
        up = np.spacing(a32).astype(np.float64)                           # to the next float away from zero
        down = a32.astype(np.float64) - np.nextafter(a32, np.float32(0)).astype(np.float64)   # (smaller at a power of two)
        room = 0.5 * np.minimum(up, np.where(down > 0, down, up)) - np.abs(m64 - m32.astype(np.float64))
        err = (n + 2) * 2.0 ** -53 * np.abs(X.astype(np.float64)).mean(axis=0)
        # a channel whose values are all multiples of q with sum |x| < 2^52 q sums exactly in fp64, in every order
        ax = np.abs(X)
        q = np.where(ax > 0, np.spacing(ax), np.float32(np.inf)).min(axis=0).astype(np.float64)
        exact = ax.astype(np.float64).sum(axis=0) < 2.0 ** 52 * q
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.where(exact | (err == 0), np.inf, room / err)
        report["min_mean_gap"] = min(report["min_mean_gap"], float(gap.min()))
    return m32


def kmeans_node(X, k, seed, path, max_iterations, report):
    """-> (centres [nc, C] float32, cluster of every point, Lloyd rounds, capped)"""
    picks = seed_node(X, k, seed, path, report)
    centres = X[picks].copy()
    assign = _assign(X, centres, report)
    t = 1
    while True:
        if max_iterations > 0 and t >= max_iterations:
            return centres, assign, t, True
        t += 1
        centres = centres.copy()
        for c in range(centres.shape[0]):
            members = X[assign == c]
            if members.shape[0]:
                centres[c] = mean_f32(members, report)
            else:
                report["emptied"] += 1                      # an emptied cluster keeps its centre
        new = _assign(X, centres, report)
        mismatch = int((new != assign).sum())
        assign = new
        rate = np.float32(mismatch) / np.float32(X.shape[0])
        if float(rate) < 1.0e-3:
            return centres, assign, t, False


def build(desc, doc_begin, k, L, seed=0, weighting=TF_IDF, max_iterations=100, scoring=0):
    """desc [C, M] float32 -> dict(parent, descriptors, weight, word_id, n_nodes, n_words, C, k, L, scoring, weighting:
    the vocabulary; docs_with_word [n_words]; node_of_point [M]; rounds [levels], nodes [levels], kmeans_nodes [levels];
    nodes_capped; min_margin, min_mean_gap, min_cut_gap, picks; emptied: clusters that lost every point in some round; node_picks:
    per k-means node (path, the positions its seeding picked))"""
    X = np.ascontiguousarray(np.asarray(desc, np.float32).T)
    M, C = X.shape
    parent, rows = [-1], [np.zeros(C, np.float32)]
    has_children = [False]
    node_of_point = np.zeros(M, np.int32)
    rounds, nodes, km_nodes = [0] * L, [0] * L, [0] * L
    report = dict(min_mean_gap=np.inf, min_margin=np.inf, min_cut_gap=np.inf, picks=0, capped=0, emptied=0, node_picks=[])

    def step(pid, idx, level, path):
        nodes[level - 1] += 1
        if idx.size <= k:
            centres = X[idx].copy()
            groups = [idx[i:i + 1] for i in range(idx.size)]
        else:
            km_nodes[level - 1] += 1
            centres, assign, t, capped = kmeans_node(X[idx], k, seed, path, max_iterations, report)
            rounds[level - 1] = max(rounds[level - 1], t)
            report["capped"] += int(capped)
            groups = [idx[assign == c] for c in range(centres.shape[0])]     # ascending training order
        ids = list(range(len(parent), len(parent) + len(groups)))
        for c in centres:
            parent.append(pid)
            rows.append(c)
            has_children.append(False)
        has_children[pid] = True
        for i, g in enumerate(groups):
            if level < L and g.size > 1:
                step(ids[i], g, level + 1, path + [i])
            else:
                node_of_point[g] = ids[i]

    step(0, np.arange(M), 1, [])
    n = len(parent)
    word_id = np.full(n, -1, np.int32)
    leaves = [i for i in range(1, n) if not has_children[i]]
    word_id[leaves] = np.arange(len(leaves))
    voc = dict(parent=np.array(parent, np.int32), descriptors=np.array(rows, np.float32), weight=np.zeros(n, np.float64),
               word_id=word_id, n_nodes=n, n_words=len(leaves), C=C, k=k, L=L, scoring=scoring, weighting=weighting)
    ni = np.zeros(len(leaves), np.int32)
    n_docs = len(doc_begin) - 1
    if weighting in (TF_IDF, IDF):
        words = bow_ref.walk(voc, X.T)["word"]
        for d in range(n_docs):
            ni[np.unique(words[int(doc_begin[d]):int(doc_begin[d + 1])])] += 1
        with np.errstate(divide="ignore"):
            w = np.where(ni > 0, np.log(float(n_docs) / ni.astype(np.float64)), 0.0)
    else:
        w = np.ones(len(leaves))
    voc["weight"][leaves] = w
    levels = max([l + 1 for l in range(L) if nodes[l]] or [0])
    voc.update(docs_with_word=ni, node_of_point=node_of_point, rounds=rounds, nodes=nodes, kmeans_nodes=km_nodes, levels=levels,
               nodes_capped=report["capped"], min_margin=report["min_margin"], min_mean_gap=report["min_mean_gap"], min_cut_gap=report["min_cut_gap"], picks=report["picks"], emptied=report["emptied"], node_picks=report["node_picks"])
    return voc
