"""numpy restatement of the loop detector's bag of words, written from the description in include/sage_ba.h (test
infrastructure; the library shares no code with it):

  walk       every point's descent through the vocabulary tree: nearest child by sum_ch (F - desc)^2 accumulated channel by
             channel in the given dtype, the first smallest wins, a NaN distance counts as smallest (np.argmin's rule, which is
             torch.argmin's); per point the leaf, its word, and the smallest relative margin (d_second - d_best) / d_second
             met on the way
  transform  the vector of a set of words reached: weight * M per word with weight > 0, L1-normalised by the sequential
             ascending sum; and the statistics sage_bow_transform reports
  score      L1Scoring::score, sequentially over the common words in ascending order
  query      TemplatedDatabase::queryL1 over a list of vectors: sequentially (the library's doubles bit for bit), or by brute
             force over dense vectors (np.sum: another summation order, equal to ~1e-16)
"""
import numpy as np


def children_of(voc):
    """per node the list of its children, ascending node index"""
    kids = [[] for _ in range(voc["n_nodes"])]
    for i in range(1, voc["n_nodes"]):
        kids[int(voc["parent"][i])].append(i)
    return kids


def walk(voc, F, dtype=np.float64):
    """F [C, M] float32 -> dict(leaf [M] node index, word [M], margin [M] float64 (inf where no node on the way had a second
    child, NaN where a NaN distance decided), inner: the set of inner nodes some point passed)"""
    kids = children_of(voc)
    D = voc["descriptors"].astype(dtype)
    Fd = np.asarray(F).astype(dtype)
    C, M = Fd.shape
    node = np.zeros(M, np.int64)
    margin = np.full(M, np.inf)
    inner = set()
    todo = [(0, np.arange(M))]
    while todo:
        at, idx = todo.pop()
        ch = kids[at]
        if not ch:
            continue
        inner.add(at)
        d = np.zeros((idx.size, len(ch)), dtype)
        for c in range(C):                                     # channel by channel: one rounding per addition
            e = Fd[c, idx][:, None] - D[ch, c][None, :]
            d = d + e * e
        best = np.argmin(d, axis=1)
        if len(ch) > 1:
            s = np.sort(d.astype(np.float64), axis=1)          # NaNs sort last
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.where(s[:, 1] > 0, (s[:, 1] - s[:, 0]) / s[:, 1], 0.0)
            m = np.where(np.isnan(d).any(axis=1), np.nan, m)
            margin[idx] = np.minimum(margin[idx], m)           # (a NaN stays)
        for j, c in enumerate(ch):
            sub = idx[best == j]
            if sub.size:
                node[sub] = c
                todo.append((c, sub))
    return dict(leaf=node, word=voc["word_id"][node].astype(np.int32), margin=margin, inner=inner)


def transform(voc, words, M):
    """the vector of the words reached (``words``: any array of word ids, e.g. walk()["word"]) for M points
    -> (ids int32 [n], values float64 [n], stats dict)"""
    hit = np.unique(np.asarray(words))
    leaf_of_word = np.full(voc["n_words"], -1, np.int64)
    leaves = np.nonzero(voc["word_id"] >= 0)[0]
    leaf_of_word[voc["word_id"][leaves]] = leaves
    ids, vals = [], []
    norm = 0.0
    for w in hit:                                              # ascending
        weight = float(voc["weight"][leaf_of_word[w]])
        if weight > 0:
            ids.append(int(w))
            vals.append(weight * float(M))
            norm += abs(vals[-1])
    if norm > 0.0:
        vals = [v / norm for v in vals]
    inner = set()
    for w in hit:
        p = int(voc["parent"][leaf_of_word[w]])
        while p >= 0 and p not in inner:
            inner.add(p)
            p = int(voc["parent"][p])
    stats = dict(n_points=int(M), n_words=len(ids), n_leaves_hit=int(hit.size), n_zero_weight=int(hit.size) - len(ids),
                 n_inner_nodes_hit=len(inner))
    return np.array(ids, np.int32), np.array(vals, np.float64), stats


def l1_value(ids1, vals1, ids2, vals2):
    """sum over the common words, ascending, of |v - w| - |v| - |w| -> (the sum, whether there is a common word)"""
    w = dict(zip((int(i) for i in ids2), (float(v) for v in vals2)))
    s, any_common = 0.0, False
    for i, v in zip(ids1, vals1):
        if int(i) in w:
            term = abs(float(v) - w[int(i)]) - abs(float(v)) - abs(w[int(i)])
            s = s + term if any_common else term
            any_common = True
    return s, any_common


def score(ids1, vals1, ids2, vals2):
    return -l1_value(ids1, vals1, ids2, vals2)[0] / 2.0


def dense(ids, vals, n_words):
    v = np.zeros(n_words)
    v[np.asarray(ids, np.int64)] = vals
    return v


def query(entries, ids, vals, n_words, max_results=0, max_id=-1, brute=False):
    """entries: list of (ids, vals) in the order they were added -> (entry ids, scores), best first, ties by ascending id"""
    found = []
    q = dense(ids, vals, n_words)
    for e, (eids, evals) in enumerate(entries):
        if not (e < max_id or max_id == -1):
            continue
        value, common = l1_value(ids, vals, eids, evals)          # (the query's words in ascending order)
        if not common:
            continue
        if brute:
            w = dense(eids, evals, n_words)
            value = float(np.sum(np.abs(q - w) - np.abs(q) - np.abs(w)))
        found.append((value, e))
    found.sort()
    if max_results > 0:
        found = found[:max_results]
    return np.array([e for _, e in found], np.int32), np.array([-v / 2.0 for v, _ in found], np.float64)
