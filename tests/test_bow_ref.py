"""CPU tests of the loop detector's bag of words (no GPU): the vocabulary loader on the shipped file, the numpy restatement
(tests/bow_ref.py) against a literal torch-CPU rendering of the reference's recursive expression, the guarantee the GPU test
rests on (no point of any GPU case is ambiguous), the host library (sage_bow_score, the database) through the C ABI, and the
validation of sage_vocabulary_create.

The cases of tests/test_gpu_bow.py are defined here (CASES, case()) so that both files talk about the same inputs.

Ambiguity.  A point is ambiguous when, at some node on its way, the relative margin (d_second - d_best) / d_second between
the two nearest children is below 4 (C + 2) 2^-24 in fp64.  A difference-form fp32 sum of C non-negative terms is within
(C + 2) 2^-24 relative of the exact sum in any summation order (one rounding per difference, square and addition, all terms
of one sign); two candidates further apart than twice that cannot swap, the remaining factor 2 covers the second-order
terms.  Smallest margins measured over the cases here (fp64): fixture vocabulary, C = 16 (threshold 4.3e-6): iid 48x64
3.6e-5, nodes 48x64 1.3e-4, nodes 96x128 2.4e-5; ragged C = 5 (1.7e-6): nodes 1.4e-4, iid (seed 1) 1.0e-4; k = 12, L = 4,
C = 32 (8.1e-6): 8.6e-5.  A seed with an ambiguous point is replaced by another seed (ragged iid, seed 0: one point at
4.3e-7), never the threshold.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from sage_slam_amd import capi, synth, vocabulary
from tests import bow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bow_voc.yml.gz")


@functools.lru_cache(maxsize=None)
def vocab(name):
    if name == "fixture":
        return vocabulary.load_opencv_yaml(FIXTURE)
    if name == "ragged":                      # the generic path (C = 5), fan-outs 1..12, leaves at depths 1..4, zero weights
        return synth.make_vocabulary(12, 4, 5, seed=0, ragged=True)
    if name == "big32":                       # 22 621 nodes, 2.9 MB of descriptors: the levels read from global memory
        return synth.make_vocabulary(12, 4, 32, seed=0)
    raise KeyError(name)


# name -> (vocabulary, H, W, kind, seed, the first m points only (0: all), with locations)
CASES = {
    "fix_iid48": ("fixture", 48, 64, "iid", 0, 0, True),
    "fix_nodes48": ("fixture", 48, 64, "nodes", 0, 0, True),
    "fix_nodes48_gathered": ("fixture", 48, 64, "nodes", 0, 0, False),
    "fix_m1": ("fixture", 48, 64, "nodes", 0, 1, True),
    "fix_m63": ("fixture", 48, 64, "nodes", 0, 63, True),
    "fix_m64": ("fixture", 48, 64, "nodes", 0, 64, True),
    "fix_m65": ("fixture", 48, 64, "nodes", 0, 65, True),
    "fix_m257": ("fixture", 48, 64, "nodes", 0, 257, True),
    "fix_nodes96": ("fixture", 96, 128, "nodes", 0, 0, True),
    "fix_nan": ("fixture", 48, 64, "nan", 0, 0, True),
    "fix_const": ("fixture", 48, 64, "constant", 0, 0, True),
    "ragged_nodes": ("ragged", 48, 64, "nodes", 0, 0, True),
    "ragged_iid": ("ragged", 48, 64, "iid", 1, 0, False),           # (seed 0 has one ambiguous point)
    "ragged_empty": ("ragged", 0, 0, "zero_leaf", 0, 100, False),
    "big32_nodes": ("big32", 48, 64, "nodes", 0, 0, True),
}


def zero_weight_leaf_descriptor(voc):
    """the descriptor of a leaf of weight 0 that, walked through the tree, ends on that very leaf"""
    leaves = np.nonzero((voc["word_id"] >= 0) & (voc["weight"] == 0))[0]
    got = ref.walk(voc, voc["descriptors"][leaves].T, np.float64)
    own = np.nonzero(got["leaf"] == leaves)[0]
    assert own.size, "no zero-weight leaf is its own nearest leaf"
    return voc["descriptors"][leaves[own[0]]]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(voc, desc [C, P], loc1d [M] or None, M, P, F [C, M] the gathered descriptors, w64 / w32: bow_ref.walk in
    fp64 / fp32, ids, vals, stats: bow_ref.transform of the fp64 words).  Computed once and shared: do not write into it."""
    vname, H, W, kind, seed, first, with_loc = CASES[name]
    voc = vocab(vname)
    if kind == "zero_leaf":
        F = np.repeat(zero_weight_leaf_descriptor(voc)[:, None], first, axis=1).astype(np.float32)
        desc, loc = F, None
    else:
        prob = synth.make_bow_problem(H, W, voc["C"], seed, kind, voc)
        loc = prob["loc1d"][:first] if first else prob["loc1d"]
        F = np.ascontiguousarray(prob["desc"][:, loc])
        desc = prob["desc"]
        if not with_loc:
            desc, loc = F, None
    M = F.shape[1]
    w64, w32 = ref.walk(voc, F, np.float64), ref.walk(voc, F, np.float32)
    ids, vals, stats = ref.transform(voc, w64["word"], M)
    return dict(voc=voc, vname=vname, desc=desc, loc1d=loc, M=M, P=desc.shape[1], F=F, w64=w64, w32=w32, ids=ids, vals=vals, stats=stats)


def threshold(Cn):
    return 4.0 * (Cn + 2) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. the loader
def test_loader_reads_the_shipped_vocabulary():
    v = vocab("fixture")
    assert (v["k"], v["L"], v["C"], v["scoring"], v["weighting"]) == (10, 3, 16, 0, 0)
    assert v["n_nodes"] == 1111 and v["n_words"] == 1000                      # 1 110 nodes plus the root
    assert v["descriptors"].shape == (1111, 16) and v["descriptors"].dtype == np.float32 and not v["descriptors"][0].any()
    fan = np.bincount(v["parent"][1:], minlength=1111)
    assert set(fan) == {0, 10} and (fan == 10).sum() == 111                   # the root and the 110 inner nodes below it
    inner = np.nonzero(fan[1:] > 0)[0] + 1
    assert inner.size == 110 and not v["weight"][inner].any() and (v["word_id"][inner] == -1).all()
    leaves = np.nonzero(fan == 0)[0]
    assert np.array_equal(np.sort(v["word_id"][leaves]), np.arange(1000)) and (v["weight"][leaves] > 0).all()
    assert v["parent"][0] == -1 and (v["parent"][1:] < np.arange(1, 1111)).all() and (v["parent"][1:] >= 0).all()
    assert v["descriptors"][1, 0] == np.float32(-0.399843) and v["weight"][30] == 1.4515348829882915e+00
    assert v["parent"][30] == 11 and v["word_id"][30] == 9


def test_loader_refuses_children_out_of_order(tmp_path):
    head = "%YAML:1.0\n---\nvocabulary:\n   k: 2\n   L: 1\n   scoringType: 0\n   weightingType: 0\n   nodes:\n"
    node = '      - {{ nodeId:{}, parentId:0, weight:1.,\n          descriptor:"0.5 0.25 " }}\n'
    words = "   words:\n      - { wordId:0, nodeId:1 }\n      - { wordId:1, nodeId:2 }\n"
    good = tmp_path / "good.yml"
    good.write_text(head + node.format(1) + node.format(2) + words)
    v = vocabulary.load_opencv_yaml(str(good))
    assert v["n_nodes"] == 3 and v["C"] == 2 and v["descriptors"][2].tolist() == [0.5, 0.25] and v["word_id"].tolist() == [-1, 0, 1]
    bad = tmp_path / "bad.yml"
    bad.write_text(head + node.format(2) + node.format(1) + words)
    with pytest.raises(ValueError, match="ascending"):
        vocabulary.load_opencv_yaml(str(bad))
    with pytest.raises(ValueError):
        vocabulary.load_opencv_yaml(__file__)


# ------------------------------------------------------------------------------------------------ 2. the literal expression
def torch_transform(voc, F):
    """the reference's transform / subset_transform (tensor_vocabulary.cpp:131-245) operation by operation with torch on
    the CPU: index, broadcast subtraction, square, sum, argmin, nonzero, recursion; then BowVector::normalize (L1)"""
    import torch
    kids = ref.children_of(voc)
    node_desc = torch.from_numpy(voc["descriptors"].T.copy())                 # C x N
    features = torch.from_numpy(np.ascontiguousarray(F))
    v = {}

    def descend(sub, idx, at):
        ch = torch.tensor(kids[at], dtype=torch.long)
        cd = node_desc[:, ch]
        Cn, S, K = sub.size(0), sub.size(1), cd.size(1)
        dist = torch.sum(torch.square(sub.reshape(Cn, S, 1) - cd.reshape(Cn, 1, K)), 0, False)
        cl = torch.argmin(dist, 1, False).to(torch.long)
        for i in range(K):
            within = torch.nonzero(cl == i).reshape(-1)
            if within.size(0) >= 1:
                subset(within if idx is None else idx[within], int(ch[i].item()))

    def subset(idx, at):
        if not kids[at]:
            w = float(voc["weight"][at])
            if w > 0:
                word = int(voc["word_id"][at])
                v[word] = v.get(word, 0.0) + w * features.size(1)
            return
        descend(features[:, idx], idx, at)

    descend(features, None, 0)
    ids = sorted(v)
    norm = 0.0
    for i in ids:
        norm += abs(v[i])
    if norm > 0.0:
        for i in ids:
            v[i] /= norm
    return np.array(ids, np.int32), np.array([v[i] for i in ids], np.float64)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_literal_torch_expression(name):
    c = case(name)
    ids, vals = torch_transform(c["voc"], c["F"])
    assert np.array_equal(ids, c["ids"]) and ids.dtype == c["ids"].dtype
    assert vals.tobytes() == c["vals"].tobytes()
    ids32, vals32, stats32 = ref.transform(c["voc"], c["w32"]["word"], c["M"])
    assert np.array_equal(ids32, ids) and vals32.tobytes() == vals.tobytes() and stats32 == c["stats"]
    if ids.size:
        assert abs(vals.sum() - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. no ambiguous point
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases_have_no_ambiguous_point(name):
    c = case(name)
    thr = threshold(c["voc"]["C"])
    m = c["w64"]["margin"]
    n_amb = int((m < thr).sum())                                              # (a NaN margin: a NaN decided, by rule)
    finite = m[np.isfinite(m)]
    print(f"{name}: M {c['M']} words {c['stats']['n_leaves_hit']} written {c['stats']['n_words']} inner {c['stats']['n_inner_nodes_hit']} "
          f"smallest margin {finite.min() if finite.size else float('nan'):.2e} threshold {thr:.2e} ambiguous {n_amb}")
    assert n_amb == 0
    assert np.array_equal(c["w32"]["word"], c["w64"]["word"])                 # fp32 agrees with fp64 on every point
    assert c["stats"]["n_inner_nodes_hit"] == len(c["w64"]["inner"])          # two ways to count them


def test_cases_cover_what_they_are_meant_to():
    fan = lambda v: np.bincount(v["parent"][1:], minlength=v["n_nodes"])
    r = vocab("ragged")
    f = fan(r)
    depth = np.zeros(r["n_nodes"], int)
    for i in range(1, r["n_nodes"]):
        depth[i] = depth[r["parent"][i]] + 1
    assert set(f[f > 0]) == set(range(1, 13)) and set(depth[f == 0]) == {1, 2, 3, 4} and r["C"] == 5
    assert ((r["weight"] == 0) & (f == 0)).sum() > 0
    b = vocab("big32")
    assert b["n_nodes"] == 22621 and b["C"] == 32 and b["descriptors"].nbytes > 2.8e6
    assert case("fix_iid48")["M"] == 1536 and case("fix_nodes96")["M"] == 8960
    assert case("fix_nodes48")["stats"]["n_words"] > 500 > case("fix_iid48")["stats"]["n_words"] > 50
    assert case("ragged_nodes")["stats"]["n_zero_weight"] > 0
    e = case("ragged_empty")
    assert e["stats"] == dict(n_points=100, n_words=0, n_leaves_hit=1, n_zero_weight=1, n_inner_nodes_hit=e["stats"]["n_inner_nodes_hit"])
    assert e["ids"].size == 0
    n = case("fix_nan")
    kids = ref.children_of(n["voc"])
    first_leaf = 0
    while kids[first_leaf]:
        first_leaf = kids[first_leaf][0]
    assert (n["w64"]["leaf"] == first_leaf).all() and n["stats"]["n_leaves_hit"] == 1
    k = case("fix_const")
    assert k["stats"]["n_words"] == 1 and k["vals"].tolist() == [1.0]


@functools.lru_cache(maxsize=None)
def retrieval_keyframes():
    """the twelve keyframes of the end-to-end GPU test: 0..10 are different scenes, 11 revisits keyframe 2 (its descriptors
    plus a little noise) -> list of dict(desc, loc1d, M, w64, ids, vals) on the shipped vocabulary.  Shared: do not write."""
    v = vocab("fixture")
    probs = [synth.make_bow_problem(48, 64, 16, seed=112 + k, kind="iid" if k % 3 == 0 else "nodes", voc=v) for k in range(11)]   # (seeds 100, 111: an ambiguous point)
    again = dict(probs[2])
    again["desc"] = (probs[2]["desc"] + np.random.default_rng(7).normal(0.0, 0.01, probs[2]["desc"].shape)).astype(np.float32)
    probs.append(again)
    out = []
    for p in probs:
        w64 = ref.walk(v, p["desc"][:, p["loc1d"]], np.float64)
        ids, vals, _ = ref.transform(v, w64["word"], p["M"])
        out.append(dict(desc=p["desc"], loc1d=p["loc1d"], M=p["M"], w64=w64, ids=ids, vals=vals))
    return out


def test_retrieval_keyframes_have_no_ambiguous_point_and_a_clear_answer():
    kfs = retrieval_keyframes()
    for k, kf in enumerate(kfs):
        assert int((kf["w64"]["margin"] < threshold(16)).sum()) == 0, k
    vecs = [(kf["ids"], kf["vals"]) for kf in kfs]
    e, s = ref.query(vecs, *vecs[11], 1000, 0, 11)                  # without itself: the revisited keyframe comes first
    print("query of keyframe 11 among 0..10:", e.tolist(), np.round(s, 4).tolist())
    assert e[0] == 2 and s[0] > s[1]


# ------------------------------------------------------------------------------------------------ 4. the host library
def random_vectors(n_words, n, seed, fill=0.15):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ids = np.nonzero(rng.random(n_words) < fill)[0].astype(np.int32)
        vals = rng.random(ids.size)
        out.append((ids, vals / vals.sum() if ids.size else vals))
    return out


def test_score_is_the_sequential_sum():
    vecs = random_vectors(200, 12, seed=1)
    for a in vecs[:6]:
        for b in vecs[6:]:
            s = capi.bow_score(a[0], a[1], b[0], b[1])
            assert s == ref.score(a[0], a[1], b[0], b[1])                                             # the same double
            da, db = ref.dense(a[0], a[1], 200), ref.dense(b[0], b[1], 200)
            assert abs(s - (1.0 - 0.5 * np.abs(da - db).sum())) < 1e-12                               # Nister's form
    a = vecs[0]
    assert capi.bow_score(a[0], a[1], a[0], a[1]) == pytest.approx(1.0, abs=1e-15)
    assert capi.bow_score(a[0], a[1], [], []) == 0.0 and capi.bow_score([], [], [], []) == 0.0
    assert capi.bow_score([1, 3], [0.5, 0.5], [0, 2], [0.5, 0.5]) == 0.0                              # no common word


def test_score_rejects_bad_vectors():
    assert capi.bow_score_raw([1, 1], [0.5, 0.5], [1], [1.0])[0] == -1                                # not strictly ascending
    assert capi.bow_score_raw([2, 1], [0.5, 0.5], [1], [1.0])[0] == -1
    assert capi.bow_score_raw([1], [1.0], [-1, 2], [0.5, 0.5])[0] == -1
    assert capi.bow_score_raw([1], [float("nan")], [1], [1.0])[0] == -1
    f = capi.lib().sage_bow_score
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    one = np.array([1], np.int32); val = np.array([1.0])
    s = C.c_double()
    assert f(one.ctypes.data, val.ctypes.data, 1, one.ctypes.data, val.ctypes.data, 1, None) == -1
    assert f(None, val.ctypes.data, 1, one.ctypes.data, val.ctypes.data, 1, C.addressof(s)) == -1
    assert f(one.ctypes.data, val.ctypes.data, -1, one.ctypes.data, val.ctypes.data, 1, C.addressof(s)) == -1
    assert f(None, None, 0, one.ctypes.data, val.ctypes.data, 1, C.addressof(s)) == 0 and s.value == 0.0


def test_database_query_order_and_scores():
    n_words = 120
    vecs = random_vectors(n_words, 10, seed=2)
    vecs[7] = (vecs[3][0].copy(), vecs[3][1].copy())                           # a tie: entries 3 and 7 are the same vector
    vecs.append((np.array([n_words - 1], np.int32), np.array([1.0])))         # entry 10 ...
    q_ids, q_vals = random_vectors(n_words, 1, seed=3)[0]
    q_ids, q_vals = q_ids[q_ids != n_words - 1], q_vals[q_ids != n_words - 1]  # ... shares no word with the query
    db = capi.BowDatabase(n_words)
    try:
        assert len(db) == 0
        e, s = db.query(q_ids, q_vals)                                         # an empty database
        assert e.size == 0 and s.size == 0
        for k, (ids, vals) in enumerate(vecs):
            assert db.add(ids, vals) == k
        assert db.add([], []) == 11 and len(db) == 12                          # an entry without words
        for max_results, max_id in ((0, -1), (4, -1), (0, 7), (3, 5), (-2, -1), (0, 0), (100, 100)):
            e, s = db.query(q_ids, q_vals, max_results, max_id)
            we, wsc = ref.query(vecs, q_ids, q_vals, n_words, max_results, max_id)
            assert np.array_equal(e, we) and s.tobytes() == wsc.tobytes(), (max_results, max_id)
            be, bs = ref.query(vecs, q_ids, q_vals, n_words, max_results, max_id, brute=True)
            assert np.array_equal(e, be) and np.abs(s - bs).max(initial=0.0) < 1e-12
            assert (np.diff(s) <= 0).all()                                     # best first
        e, s = db.query(q_ids, q_vals)
        sharing = [k for k, (ids, _) in enumerate(vecs) if np.intersect1d(ids, q_ids).size]
        assert sorted(e) == sharing and len(sharing) >= 8 and 10 not in e and 11 not in e   # no common word: no result
        at3, at7 = int(np.nonzero(e == 3)[0][0]), int(np.nonzero(e == 7)[0][0])
        assert at7 == at3 + 1 and s[at3] == s[at7]                             # ties by ascending entry id
        assert db.query(q_ids, q_vals, 0, 0)[0].size == 0                      # max_id = 0: every entry is skipped
        assert db.query([], [])[0].size == 0
        # the query's own vector, once added, comes first with its self-score
        me = db.add(q_ids, q_vals)
        e, s = db.query(q_ids, q_vals, 1)
        assert e.tolist() == [me] and s[0] == ref.score(q_ids, q_vals, q_ids, q_vals)
        # capacity
        rc, e, s, n = db.query_raw(q_ids, q_vals, 0, -1, capacity=3)
        assert rc == -1 and n == len(sharing) + 1
        rc, e, s, n = db.query_raw(q_ids, q_vals, 3, -1, capacity=3)
        assert rc == 0 and n == 3 and np.array_equal(e, ref.query(vecs + [([], []), (q_ids, q_vals)], q_ids, q_vals, n_words, 3)[0])
        # misuse
        assert db.add_raw([5, 4], [0.5, 0.5]) == -1 and db.add_raw([n_words], [1.0]) == -1 and db.add_raw([-1], [1.0]) == -1
        assert db.add_raw([1], [float("inf")]) == -1 and len(db) == 13
        assert db.query_raw([3, 3], [0.5, 0.5])[0] == -1 and db.query_raw([n_words], [1.0])[0] == -1
    finally:
        db.close()
    L = capi.lib()
    L.sage_bow_db_create.argtypes = [C.c_int, C.c_void_p]
    h = C.c_void_p()
    assert L.sage_bow_db_create(0, C.addressof(h)) == -1 and L.sage_bow_db_create(5, None) == -1
    L.sage_bow_db_size.argtypes = [C.c_void_p]
    assert L.sage_bow_db_size(None) == -1


def test_database_add_and_query_from_three_threads():
    """the reference adds and queries from three threads: every vector gets an id of its own, a query sees whole entries"""
    import threading
    n_words = 64
    vecs = random_vectors(n_words, 90, seed=4, fill=0.3)
    db = capi.BowDatabase(n_words)
    got = [None] * len(vecs)
    bad = []

    def work(t):
        for k in range(t, len(vecs), 3):
            got[k] = db.add(*vecs[k])
            e, s = db.query(*vecs[k], 5)
            if not (e.size >= 1 and s[0] == pytest.approx(1.0, abs=1e-12) and (np.diff(s) <= 0).all()):
                bad.append(k)
    try:
        threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
        [t.start() for t in threads]
        [t.join() for t in threads]
        assert not bad and sorted(got) == list(range(len(vecs))) and len(db) == len(vecs)
        order = np.argsort(got)                                                # the vectors in the order they were added
        e, s = db.query(*vecs[0])
        we, wsc = ref.query([vecs[k] for k in order], *vecs[0], n_words)
        assert np.array_equal(e, we) and s.tobytes() == wsc.tobytes()
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 5. validation
def small_tree():
    """root -> {1, 2}, 1 -> {3, 4}: leaves 2, 3, 4"""
    return dict(parent=np.array([-1, 0, 0, 1, 1], np.int32), descriptors=np.zeros((5, 3), np.float32),
                weight=np.array([0, 0, 1.0, 2.0, 0.5]), word_id=np.array([-1, -1, 0, 1, 2], np.int32))


def create_status(**over):
    t = {**small_tree(), **over}
    rc, h = capi.vocabulary_create_raw(t["parent"], t["descriptors"], t["weight"], t["word_id"], t.get("scoring", 0))
    assert not h.value or rc == 0
    return rc


def test_vocabulary_create_validates_the_tree_before_touching_the_device():
    """(on a machine without a GPU a VALID tree fails later, with the runtime's no-device code: these answers come first)"""
    INVALID, UNSUPPORTED = -1, -2
    assert create_status(parent=np.array([-1, 0, 0, 4, 1], np.int32)) == INVALID          # a cycle: 3 -> 4 -> ... (parent >= i)
    assert create_status(parent=np.array([-1, 1, 0, 1, 1], np.int32)) == INVALID          # a node its own parent
    assert create_status(parent=np.array([0, 0, 0, 1, 1], np.int32)) == INVALID           # the root has a parent
    assert create_status(parent=np.array([-1, -1, 0, 1, 1], np.int32)) == INVALID
    assert create_status(word_id=np.array([-1, -1, 0, 1, 3], np.int32)) == INVALID         # word 2 is missing
    assert create_status(word_id=np.array([-1, -1, 0, 1, 1], np.int32)) == INVALID         # word 1 twice
    assert create_status(word_id=np.array([-1, 3, 0, 1, 2], np.int32)) == INVALID          # an inner node with a word id
    assert create_status(word_id=np.array([-1, -1, 0, -1, 1], np.int32)) == INVALID        # a leaf without one
    assert create_status(word_id=np.array([-1, -1, 0, -2, 1], np.int32)) == INVALID
    assert create_status(scoring=6) == INVALID and create_status(scoring=-1) == INVALID
    assert create_status(descriptors=np.zeros((5, 65), np.float32)) == UNSUPPORTED        # C = 65
    for scoring in range(1, 6):                                                            # the five other DBoW2 norms
        assert create_status(scoring=scoring) == UNSUPPORTED
    wide = dict(parent=np.array([-1] + [0] * 65, np.int32), descriptors=np.zeros((66, 3), np.float32), weight=np.ones(66),
                word_id=np.array([-1] + list(range(65)), np.int32))
    assert create_status(**wide) == UNSUPPORTED                                            # a fan-out of 65
    deep = dict(parent=np.arange(-1, 9, dtype=np.int32), descriptors=np.zeros((10, 3), np.float32), weight=np.ones(10),
                word_id=np.array([-1] * 9 + [0], np.int32))
    assert create_status(**deep) == UNSUPPORTED                                            # a leaf at depth 9
    f = capi.lib().sage_vocabulary_create
    f.argtypes = [C.c_void_p, C.c_void_p]
    h = C.c_void_p()
    d = capi.SageVocabularyDesc(1, 3, 0, 0, 0, 0, 0)
    assert f(None, C.addressof(h)) == INVALID and f(C.addressof(d), C.addressof(h)) == INVALID
    L = capi.lib()
    for name in ("num_nodes", "num_words", "channels", "depth", "max_fanout", "staged_nodes"):
        fn = getattr(L, "sage_vocabulary_" + name)
        fn.argtypes = [C.c_void_p]
        assert fn(None) == -1


def test_bow_transform_checks_its_arguments_before_touching_the_device():
    """a NULL workspace, vocabulary, descriptor or output pointer answers SAGE_E_INVALID without a launch (the other
    pointers here are not real: nothing may dereference them)"""
    fake = C.create_string_buffer(64)
    p = C.addressof(fake)
    good = dict(ws=p, voc=p, desc=p, loc=None, M=4, P=4, ids=p, vals=p, cap=4, words=None, out=p)
    keys = ("ws", "voc", "desc", "loc", "M", "P", "ids", "vals", "cap", "words", "out")
    for name in ("ws", "voc", "desc", "ids", "vals", "out"):
        assert capi.bow_transform_raw(*[{**good, name: None}[k] for k in keys]) == -1, name
