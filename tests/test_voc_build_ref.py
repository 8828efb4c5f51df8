"""The vocabulary trainer's host side, no device needed: the restatement tests/voc_build_ref.py on a hand-derived tree, the
draw function and the plan of the library against the formulas of include/sage_ba.h, the argument checks, the vocabulary
file writer -- and the condition tests/test_gpu_voc_build.py rests on: in every case it runs, no point of any Lloyd round
has its two nearest centres within MARGIN_BOUND of each other, no seeding cut lies within CUT_BOUND of a running sum, and no
mean lies within the fp64 summation error of an fp32 rounding boundary (DESIGN.md derives the three).  The seeds of the
cases were searched on the CPU for that; one differing decision would change everything after it, so the cap is zero."""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

from sage_slam_amd import synth, vocabulary
from tests import voc_build_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bow_voc.yml.gz")


def margin_bound(Cn):   # two fp32 difference-form sums of C terms, each within (C + 2) 2^-24 of its fp64 value, and as much again
    return 4 * (Cn + 2) * 2.0 ** -24


def cut_bound(Cn):      # a running sum of min_d = sqrtf(d2) terms, each within ((C + 2) / 2 + 1) 2^-24; the cut scales with the total
    return 4 * (Cn + 2) * 2.0 ** -24


def _iid(Cn, M, seed, sigma=0.3):
    return np.random.default_rng(seed).normal(0.0, sigma, (Cn, M)).astype(np.float32)


def _docs(M, n_docs):
    return np.linspace(0, M, n_docs + 1).astype(np.int64)


def _generic(seed):
    return dict(desc=_iid(5, 40, 100 + seed), doc_begin=_docs(40, 4), k=3, L=2)


def _tiles(M, seed):
    d = _iid(3, M, 200 + seed)
    d[:, M - 1] += 40.0                      # far out: the seeding's cut falls on the last point, in the last tile
    b = np.array([0, M // 3, M // 3, M], np.int64)   # (an empty document)
    return dict(desc=d, doc_begin=b, k=4, L=1)


def _small_children(seed):
    rng = np.random.default_rng(300 + seed)
    a = np.array([[10.0], [0.0]]) + rng.normal(0, 0.1, (2, 3))     # three points: a child of n <= k
    b = np.array([[0.0], [10.0]]) + rng.normal(0, 0.1, (2, 1))     # one point: a leaf at level 1
    c = rng.normal(0, 0.5, (2, 8))
    d = np.concatenate([c[:, :4], a, c[:, 4:], b], axis=1).astype(np.float32)
    return dict(desc=d, doc_begin=_docs(12, 3), k=3, L=2)


def _identical(seed):
    rng = np.random.default_rng(400 + seed)
    same = np.repeat(rng.normal(0, 0.3, (3, 1)), 6, axis=1)
    others = 5.0 + rng.normal(0, 0.3, (3, 6))
    d = np.concatenate([others[:, :2], same, others[:, 2:]], axis=1).astype(np.float32)
    return dict(desc=d, doc_begin=_docs(12, 2), k=2, L=2)


def _duplicates(seed):
    base = _iid(4, 15, 500 + seed)
    return dict(desc=np.ascontiguousarray(np.concatenate([base, base], axis=1)), doc_begin=_docs(30, 3), k=3, L=1)


def _emptied(seed):
    return dict(desc=_iid(1, 20, 600 + seed, sigma=1.0), doc_begin=_docs(20, 2), k=5, L=1)


def _lds_max(seed):
    t = synth.make_voc_training_set(64, 1, 64, 4, 1024, seed=seed, kind="planted")
    return dict(desc=t["desc"], doc_begin=t["doc_begin"], k=64, L=1)


def _shipped(seed):
    t = synth.make_voc_training_set(10, 3, 16, 20, 1000, seed=seed, kind="planted")
    return dict(desc=t["desc"], doc_begin=t["doc_begin"], k=10, L=3)


def _capped(seed):
    return dict(_generic(seed), max_iterations=2)


# name -> (constructor, the seed of data and draws: searched so that the restatement alone satisfies the condition)
CASES = {
    "generic": (_generic, 123),
    "tile255": (functools.partial(_tiles, 255), 0),
    "tile256": (functools.partial(_tiles, 256), 0),
    "tile257": (functools.partial(_tiles, 257), 0),
    "tile513": (functools.partial(_tiles, 513), 1),
    "small_children": (_small_children, 1),
    "identical": (_identical, 0),
    "duplicates": (_duplicates, 2),
    "emptied": (_emptied, 980),
    "lds_max": (_lds_max, 40),
    "shipped": (_shipped, 11),
    "capped": (_capped, 21),
}


def make(name, seed):
    """-> dict(desc [C, M], doc_begin, k, L, seed, max_iterations, weighting, ref: the restatement's result)"""
    c = dict(CASES[name][0](seed))
    c.setdefault("max_iterations", 100)
    c.update(seed=seed, weighting=ref.TF_IDF, name=name)
    c["ref"] = ref.build(c["desc"], c["doc_begin"], c["k"], c["L"], seed=seed, weighting=c["weighting"],
                         max_iterations=c["max_iterations"])
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return make(name, CASES[name][1])


def decidable(c):
    r, Cn = c["ref"], c["desc"].shape[0]
    return r["min_margin"] > margin_bound(Cn) and r["min_cut_gap"] > cut_bound(Cn) and r["min_mean_gap"] > 1.0


@pytest.fixture(scope="module")
def L():
    from sage_slam_amd import capi
    return capi


def test_eight_points_give_the_hand_derived_tree():
    """C = 1, x = 0 1 2 3 100 101 102 104, k = 2, L = 2, seed 2, two documents of four points.
    Root: u(0) in [3/8, 4/8) picks x = 3; min_d = 3 2 1 0 97 98 99 101 (sum 401), the running sums 3 5 6 6 103 ..., the cut
    u(1) * 401 lies in (6, 103]: x = 100.  Round 1: {0 1 2 3} | {100 101 102 104}; round 2 assigns to the means 1.5 and
    101.75: the same clusters, 0 mismatches, stop.  Node 1 (path 0): picks x = 0 and x = 3 -> {0 1} | {2 3}, means 0.5 and
    2.5, stop at round 2.  Node 2 (path 1): picks x = 102 and x = 104 -> {100 101 102} | {104}, means 101 and 104, stop at
    round 2.  Creation order: 1 2 (root's), 3 4 (node 1's), 5 6 (node 2's); words 0..3 = nodes 3..6; every word is reached by
    exactly one of the two documents: weight log(2 / 1)."""
    x = np.array([[0, 1, 2, 3, 100, 101, 102, 104]], np.float32)
    u = [ref.unit(ref.draw(2, [], j)) for j in range(2)]
    assert int(u[0] * 8) == 3 and 6 < u[1] * 401 <= 103
    assert int(ref.unit(ref.draw(2, [0], 0)) * 4) == 0 and int(ref.unit(ref.draw(2, [1], 0)) * 4) == 2
    r = ref.build(x, [0, 4, 8], 2, 2, seed=2)
    assert r["node_picks"] == [((), (3, 4)), ((0,), (0, 3)), ((1,), (2, 3))]
    assert r["parent"].tolist() == [-1, 0, 0, 1, 1, 2, 2]
    assert r["descriptors"][:, 0].tolist() == [0.0, 1.5, 101.75, 0.5, 2.5, 101.0, 104.0]
    assert r["word_id"].tolist() == [-1, -1, -1, 0, 1, 2, 3]
    assert r["node_of_point"].tolist() == [3, 3, 4, 4, 5, 5, 5, 6]
    assert r["rounds"] == [2, 2] and r["nodes"] == [1, 2] and r["kmeans_nodes"] == [1, 2] and r["nodes_capped"] == 0
    assert r["docs_with_word"].tolist() == [1, 1, 1, 1]
    assert r["weight"].tolist() == [0, 0, 0] + [float(np.log(2.0))] * 4


def test_draw_function_matches_the_library(L):
    paths = [[], [0], [3], [0, 0], [9, 2, 63], [1, 2, 3, 4, 5, 6, 7]]
    for seed in (0, 1, 2, 0xDEADBEEF, (1 << 64) - 1):
        for path in paths:
            for j in (0, 1, 2, 9, 10, 640):
                assert L.vocabulary_build_draw(seed, path, j) == ref.draw(seed, path, j), (seed, path, j)
    assert ref.draw(0, [], 0) == ref._mix(ref._mix(ref._G) + ref._G)   # the formula of the header, spelled out once
    u = [ref.unit(ref.draw(7, [1], j)) for j in range(2000)]
    assert 0.0 <= min(u) and max(u) < 1.0 and abs(float(np.mean(u)) - 0.5) < 0.03


def plan_formula(Cn, M, k, Lv):
    Cp = 4 * ((Cn + 3) // 4)
    W = k ** Lv
    A = min(k ** (Lv - 1), max(1, M // 2))
    T = M // 256 + min(k ** (Lv - 1), max(1, M // (k + 1)))
    dev = M * (4 * Cp + 8 + 4 + 4 + 4 + 4 + 4) + 8 * A * k * Cp + 4 * A + T * (8 * k * Cn + 4 * k + 4 * k + 4 + 8) + 4 * W + 16 + 2 ** 24
    pin = 32 * A + 8 * T + 16 * A + 4 * A * k + 4 * A * k + 4 * A * k * Cp
    return dict(device_bytes=dev, pinned_bytes=pin, launches_per_seed_round=2, launches_per_lloyd_round=2)


@pytest.mark.parametrize("shape", [(16, 30000, 10, 3), (16, 300000, 10, 4), (5, 40, 3, 2), (64, 4096, 64, 1), (1, 1, 2, 1),
                                   (3, 513, 4, 1), (64, (1 << 31) - 1, 2, 8), (17, 1000, 32, 4)])
def test_plan_equals_the_header_formulas(L, shape):
    rc, p = L.vocabulary_build_plan_raw(*shape)
    assert rc == 0 and p == plan_formula(*shape)


def test_argument_checks_answer_without_a_device(L):
    INVALID, UNSUPPORTED = -1, -2
    plan = L.vocabulary_build_plan_raw
    assert [plan(*s)[0] for s in ((0, 10, 2, 1), (4, 0, 2, 1), (4, 10, 1, 1), (4, 10, 2, 0), (-1, 10, 2, 1))] == [INVALID] * 5
    assert [plan(*s)[0] for s in ((65, 10, 2, 1), (4, 10, 65, 1), (4, 10, 2, 9), (4, 10, 33, 4), (4, 1 << 31, 2, 1))] == [UNSUPPORTED] * 5
    assert plan(4, 10, 32, 4)[0] == 0                                            # 32^4 = 2^20 words exactly
    f = L.lib().sage_vocabulary_build_plan                                       # every output pointer may be NULL
    f.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 4
    assert f(4, 10, 2, 1, None, None, None, None) == 0
    cfg = L.vocabulary_build_config_default()
    assert (cfg.k, cfg.L, cfg.weighting, cfg.scoring, cfg.max_iterations, cfg.seed) == (10, 4, 0, 0, 100, 0)
    # sage_vocabulary_build: nothing is dereferenced but the configuration and the offsets before the checks are through
    dummy = (C.c_char * 64)()
    p = C.addressof(dummy)
    out = C.c_void_p()

    def build(ws=p, cfg_=None, desc=p, Cn=4, M=10, docs=(0, 4, 10), nd=None, o=None, **kw):
        c = L.vocabulary_build_config_default()
        c.k, c.L = 2, 2
        for name, v in kw.items():
            setattr(c, name, v)
        b = None if docs is None else np.array(docs, np.int64)
        return L.vocabulary_build_raw(ws, None if cfg_ == "null" else C.addressof(c), desc, Cn, M, None if b is None else b.ctypes.data,
                                      (len(docs) - 1 if docs is not None else 1) if nd is None else nd,
                                      None if o == "null" else C.addressof(out))

    assert build(ws=None) == INVALID and build(cfg_="null") == INVALID and build(desc=None) == INVALID
    assert build(docs=None) == INVALID and build(o="null") == INVALID
    assert build(k=1) == INVALID and build(L=0) == INVALID and build(Cn=0) == INVALID and build(M=0, docs=(0, 0)) == INVALID
    assert build(nd=0) == INVALID and build(max_iterations=-1) == INVALID
    assert build(docs=(1, 4, 10)) == INVALID and build(docs=(0, 4, 9)) == INVALID and build(docs=(0, 11, 10)) == INVALID
    assert build(weighting=4) == INVALID and build(weighting=-1) == INVALID and build(scoring=6) == INVALID and build(scoring=-1) == INVALID
    assert build(Cn=65) == UNSUPPORTED and build(k=65) == UNSUPPORTED and build(L=9) == UNSUPPORTED and build(k=33, L=4) == UNSUPPORTED
    assert out.value is None
    g = L.lib().sage_vocabulary_build_desc
    g.argtypes = [C.c_void_p, C.c_void_p]
    assert g(None, p) == INVALID and g(p, None) == INVALID


def _same(a, b):
    for key in ("parent", "descriptors", "weight", "word_id"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    for key in ("k", "L", "scoring", "weighting", "n_nodes", "n_words", "C"):
        assert a[key] == b[key], key


def test_saved_fixture_loads_back_array_for_array(tmp_path):
    v = vocabulary.load_opencv_yaml(FIXTURE)
    for name in ("a.yml.gz", "a.yml"):
        p = str(tmp_path / name)
        vocabulary.save_opencv_yaml(v, p)
        raw = open(p, "rb").read()
        assert (raw[:2] == b"\x1f\x8b") == name.endswith(".gz")
        _same(v, vocabulary.load_opencv_yaml(p))
    # with the precision of FTensor::toString the text is the committed file's, byte for byte
    p = str(tmp_path / "six.yml.gz")
    vocabulary.save_opencv_yaml(v, p, digits=6)
    assert gzip.decompress(open(p, "rb").read()) == gzip.decompress(open(FIXTURE, "rb").read())


def test_saved_ragged_vocabulary_keeps_every_bit(tmp_path):
    v = synth.make_vocabulary(5, 4, 7, seed=3, ragged=True)
    v["weighting"], v["scoring"] = 2, 0
    p = str(tmp_path / "ragged.yml")
    vocabulary.save_opencv_yaml(v, p, digits=9)
    w = vocabulary.load_opencv_yaml(p)
    _same(v, w)
    assert v["descriptors"].tobytes() == w["descriptors"].tobytes() and v["weight"].tobytes() == w["weight"].tobytes()
    text = open(p).read()
    assert text.startswith("%YAML:1.0\n---\nvocabulary:\n")
    for name, rx in vocabulary._HEADER.items():
        assert rx.search(text), name
    nodes = vocabulary._NODE.findall(text[:text.find("\n   words:")])
    words = vocabulary._WORD.findall(text[text.find("\n   words:"):])
    assert len(nodes) == v["n_nodes"] - 1 and len(words) == v["n_words"]
    assert [int(t[0]) for t in words] == list(range(v["n_words"]))
    # the order of DBoW2's save: the children of one parent together, ascending; the parent taken next is the LAST child
    # listed so far that has children and has not been taken (its parents stack)
    listed = [(int(t[0]), int(t[1])) for t in nodes]
    has_kids = set(int(q) for q in v["parent"][1:])
    stack, at = [0], 0
    while stack:
        pid = stack.pop()
        kids = [i for i in range(1, v["n_nodes"]) if v["parent"][i] == pid]
        assert listed[at:at + len(kids)] == [(c, pid) for c in kids]
        at += len(kids)
        stack += [c for c in kids if c in has_kids]
    assert at == len(listed)
    with pytest.raises(ValueError):
        vocabulary.save_opencv_yaml(dict(v, word_id=np.where(v["word_id"] == 0, 1, v["word_id"])), p)
    lossy = str(tmp_path / "six.yml")
    vocabulary.save_opencv_yaml(v, lossy, digits=6)
    assert np.allclose(vocabulary.load_opencv_yaml(lossy)["descriptors"], v["descriptors"], rtol=1e-5, atol=0)


def test_training_sets():
    t = synth.make_voc_training_set(3, 2, 5, 4, 10, seed=1, kind="planted")
    assert t["desc"].shape == (5, 40) and t["desc"].dtype == np.float32 and t["doc_begin"].tolist() == [0, 10, 20, 30, 40]
    assert np.array_equal(t["desc"], synth.make_voc_training_set(3, 2, 5, 4, 10, seed=1)["desc"])
    assert not np.array_equal(t["desc"], synth.make_voc_training_set(3, 2, 5, 4, 10, seed=2)["desc"])
    i = synth.make_voc_training_set(3, 2, 5, 4, 10, seed=1, kind="iid")
    assert i["desc"].shape == (5, 40) and 0.2 < float(i["desc"].std()) < 0.4
    # planted: the restatement finds the 3 x 3 planted leaves
    r = ref.build(t["desc"], t["doc_begin"], 3, 2, seed=1)
    assert r["n_words"] >= 9


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_cases_are_decidable(name):
    """The condition tests/test_gpu_voc_build.py rests on, and that every case exercises what it is there for."""
    c = case(name)
    r, Cn = c["ref"], c["desc"].shape[0]
    print(name, "margin %.3g (bound %.3g)  cut gap %.3g (bound %.3g)  mean gap %.3g  picks %d rounds %s nodes %s" %
          (r["min_margin"], margin_bound(Cn), r["min_cut_gap"], cut_bound(Cn), r["min_mean_gap"], r["picks"], r["rounds"], r["nodes"]))
    assert r["min_margin"] > margin_bound(Cn)
    assert r["min_cut_gap"] > cut_bound(Cn)
    assert r["min_mean_gap"] > 1.0
    kids = np.bincount(r["parent"][1:], minlength=r["n_nodes"])
    size = np.bincount(r["node_of_point"], minlength=r["n_nodes"])           # points on every leaf
    if name.startswith("tile"):
        M = c["desc"].shape[1]
        assert max(r["node_picks"][0][1]) == M - 1                          # a pick in the last tile (its last position)
        assert r["kmeans_nodes"] == [1]
    if name == "small_children":
        level1 = [i for i in range(1, r["n_nodes"]) if r["parent"][i] == 0]
        assert any(kids[i] == 0 and size[i] == 1 for i in level1)           # exactly one point: a leaf at level 1
        assert any(0 < kids[i] <= 3 and all(kids[j] == 0 and size[j] == 1 for j in range(r["n_nodes"]) if r["parent"][j] == i)
                   for i in level1) and r["nodes"][1] > r["kmeans_nodes"][1]  # n <= k: one child per point
    if name == "identical":
        assert any(kids[i] == 1 for i in range(1, r["n_nodes"]))            # dist_sum = 0: one centre, fewer than k children
    if name == "duplicates":
        assert r["n_words"] == 3 and r["picks"] == 2
    if name == "emptied":
        assert r["emptied"] >= 1 and int((size[1:] == 0).sum()) >= 1        # a leaf no point is on
    if name == "lds_max":
        assert kids[0] == 64
    if name == "shipped":
        assert r["n_words"] == 1000 and r["n_nodes"] == 1111
    if name == "capped":
        assert r["nodes_capped"] >= 1 and max(r["rounds"]) == 2
    else:
        assert r["nodes_capped"] == 0
