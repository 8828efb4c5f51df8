"""sage_bow_transform (TemplatedTensorVocabulary::transform of LoopDetector::AddKeyframe on the device) against the fp64
restatement of tests/bow_ref.py, and the retrieval end to end.

Cases (tests/test_bow_ref.py::CASES): the shipped vocabulary (k = 10, L = 3, C = 16: the whole tree is staged in LDS) at
48x64 under the eroded mask (M = 1536: six workgroups, scattered locations), the same points pre-gathered, the first
M = 1, 63, 64, 65, 257 points, 96x128 (M = 8960, every one of the 1000 words), a NaN channel (child 0 at every level), one
descriptor everywhere (one word, value exactly 1.0); a ragged C = 5 vocabulary (the generic path, fan-outs 1..12, leaves at
depths 1..4, zero weights, a vector that comes back empty); a k = 12, L = 4, C = 32 vocabulary of 22 621 nodes (levels 3 and
4 are read from global memory).

Bound: none is needed.  tests/test_bow_ref.py::test_gpu_cases_have_no_ambiguous_point shows that no point of any case has
two children within 4 (C + 2) 2^-24 of each other at any node, so every fp32 difference-form sum, in any order, makes the
decisions of fp64: the word of EVERY point is compared for equality (leave-out cap: zero points), and with the words the
vector's ids, its values (bit for bit: they are a function of the set of words) and every statistic.

Measured on an MI355X: in every case 0 of M points on another word than fp64 (M = 1 ... 8960; 1 to 1495 words reached, 3 to 1217
inner nodes passed), ids, values and statistics equal; the whole file runs in about 3 s."""
import ctypes as C

import numpy as np
import pytest

from tests import bow_ref as ref
from tests.test_bow_ref import CASES, case, vocab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def vocs(capi):
    made = {name: capi.Vocabulary(vocab(name)) for name in ("fixture", "ragged", "big32")}
    yield made
    for v in made.values():
        v.close()


def dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(capi, ws, voc, c):
    """-> (ids, vals, stats, words of the points as a host array)"""
    loc = None if c["loc1d"] is None else dev(c["loc1d"], np.int64)
    ids, vals, st, words = capi.bow_transform(ws, voc, dev(c["desc"]), loc, per_point=True)
    return ids, vals, st, words.cpu().numpy()


def raw(r):
    return r[0].tobytes() + r[1].tobytes() + bytes(memoryview(r[2])) + r[3].tobytes()


def stats_dict(st):
    return {k: getattr(st, k) for k in ("n_points", "n_words", "n_leaves_hit", "n_zero_weight", "n_inner_nodes_hit")}


def test_vocabulary_accessors(capi, vocs):
    f, r, b = vocs["fixture"], vocs["ragged"], vocs["big32"]
    assert (f.num_nodes, f.num_words, f.channels, f.depth, f.max_fanout) == (1111, 1000, 16, 3, 10)
    assert f.staged_nodes == 1111                                    # the shipped vocabulary fits the LDS budget whole
    v = vocab("ragged")
    assert (r.num_nodes, r.num_words, r.channels, r.depth, r.max_fanout) == (v["n_nodes"], v["n_words"], 5, 4, 12)
    assert r.staged_nodes == v["n_nodes"]
    assert (b.num_nodes, b.num_words, b.channels, b.depth, b.max_fanout) == (22621, 20736, 32, 4, 12)
    assert b.staged_nodes == 1 + 12 + 144                            # levels 0..2; levels 3 and 4 are read from global memory


@pytest.mark.parametrize("name", list(CASES))
def test_words_vector_and_stats_equal_the_restatement(capi, ws, vocs, name):
    c = case(name)
    ids, vals, st, words = run(capi, ws, vocs[c["vname"]], c)
    wrong = int((words != c["w64"]["word"]).sum())
    print(f"{name}: M {c['M']} points on another word than fp64: {wrong}; {stats_dict(st)}")
    assert wrong == 0
    assert ids.dtype == np.int32 and np.array_equal(ids, c["ids"])
    assert vals.tobytes() == c["vals"].tobytes()
    assert stats_dict(st) == c["stats"]


def test_special_vectors(capi, ws, vocs):
    ids, vals, st, words = run(capi, ws, vocs["fixture"], case("fix_const"))
    assert ids.size == 1 and vals.tolist() == [1.0] and (words == ids[0]).all()
    ids, vals, st, words = run(capi, ws, vocs["ragged"], case("ragged_empty"))
    assert ids.size == 0 and vals.size == 0 and (st.n_words, st.n_leaves_hit, st.n_zero_weight) == (0, 1, 1)
    ids, vals, st, words = run(capi, ws, vocs["fixture"], case("fix_nan"))
    assert st.n_leaves_hit == 1 and st.n_inner_nodes_hit == 3 and vals.tolist() == [1.0]


@pytest.mark.parametrize("name", ["fix_nodes48", "fix_nodes96", "ragged_nodes", "big32_nodes"])
def test_two_calls_return_the_same_bytes(capi, ws, vocs, name):
    c = case(name)
    voc = vocs[c["vname"]]
    a, b = run(capi, ws, voc, c), run(capi, ws, voc, c)
    assert raw(a) == raw(b)
    w2 = capi.Workspace()                                           # two workspaces share one vocabulary
    try:
        assert raw(run(capi, w2, voc, c)) == raw(a)
    finally:
        w2.close()


def test_gathered_descriptors_and_map_with_locations_agree(capi, ws, vocs):
    a, b = run(capi, ws, vocs["fixture"], case("fix_nodes48")), run(capi, ws, vocs["fixture"], case("fix_nodes48_gathered"))
    assert raw(a) == raw(b)


def test_a_call_is_unaffected_by_the_one_before(capi, vocs):
    """many words, then few, then another vocabulary with more words, then the first again, on ONE workspace: every result
    equals that of a fresh workspace (the flags were cleared; a larger vocabulary gets flags of its own)"""
    order = ["fix_nodes96", "fix_m1", "fix_iid48", "big32_nodes", "ragged_empty", "fix_m63", "fix_nodes96"]

    def fresh(c):
        w = capi.Workspace()
        try:
            return run(capi, w, vocs[c["vname"]], c)
        finally:
            w.close()

    one = capi.Workspace()
    try:
        for name in order:
            c = case(name)
            got = run(capi, one, vocs[c["vname"]], c)
            assert raw(got) == raw(fresh(c)), name
            assert np.array_equal(got[0], c["ids"]), name
    finally:
        one.close()


def test_misuse(capi, ws, vocs):
    """every SAGE_E_INVALID case returns at once (the output struct is untouched), and a valid call still works after them"""
    c = case("fix_nodes48")
    voc = vocs["fixture"]
    desc, loc = dev(c["desc"]), dev(c["loc1d"], np.int64)
    gathered = dev(c["F"])
    cap = min(c["M"], voc.num_words)
    ids = np.empty(cap, np.int32); vals = np.empty(cap, np.float64)
    out = capi.SageBowStats()
    out.n_points = -7
    good = dict(ws=ws.h, voc=voc.h, desc=capi.dptr(desc), loc=capi.dptr(loc), M=c["M"], P=c["P"], ids=ids.ctypes.data,
                vals=vals.ctypes.data, cap=cap, words=None, out=C.addressof(out))
    keys = ("ws", "voc", "desc", "loc", "M", "P", "ids", "vals", "cap", "words", "out")
    call = lambda **kw: capi.bow_transform_raw(*[{**good, **kw}[k] for k in keys])
    bad = [dict(ws=None), dict(voc=None), dict(desc=None), dict(ids=None), dict(vals=None), dict(out=None), dict(M=0), dict(M=-3),
           dict(P=0), dict(cap=cap - 1), dict(cap=0),
           dict(loc=None),                                                       # gathered descriptors need P == M
           dict(loc=None, desc=capi.dptr(gathered), M=c["M"], P=c["M"] + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert out.n_points == -7
    assert call(M=5, cap=5) == 0 and out.n_points == 5                          # capacity min(M, n_words) is enough
    assert call() == 0
    assert np.array_equal(ids[:out.n_words], c["ids"]) and vals[:out.n_words].tobytes() == c["vals"].tobytes()
    assert stats_dict(out) == c["stats"]


def test_retrieval_end_to_end(capi, ws, vocs):
    """LoopDetector::AddKeyframe twelve times, then DetectLoop's two uses of the vectors: the score against a neighbour and
    the database query -- ranking and scores equal bow_ref's on the same descriptors (the keyframes, and that none of their
    points is ambiguous: tests/test_bow_ref.py::retrieval_keyframes)"""
    from tests.test_bow_ref import retrieval_keyframes
    voc, kfs = vocs["fixture"], retrieval_keyframes()
    want = [(kf["ids"], kf["vals"]) for kf in kfs]
    db = capi.BowDatabase(voc.num_words)
    got = []
    try:
        for k, kf in enumerate(kfs):
            ids, vals, st = capi.bow_transform(ws, voc, dev(kf["desc"]), dev(kf["loc1d"], np.int64))
            assert np.array_equal(ids, kf["ids"]) and vals.tobytes() == kf["vals"].tobytes(), k
            assert db.add(ids, vals) == k
            got.append((ids, vals))
        q = got[11]
        assert capi.bow_score(*got[10], *q) == ref.score(*want[10], *want[11])
        for max_results, max_id in ((0, -1), (5, -1), (0, 11), (3, 11)):
            e, s = db.query(*q, max_results, max_id)
            we, wsc = ref.query(want, *want[11], voc.num_words, max_results, max_id)
            print(f"query(max_results {max_results}, max_id {max_id}): {e.tolist()} {np.round(s, 4).tolist()}")
            assert np.array_equal(e, we) and s.tobytes() == wsc.tobytes()
        e, s = db.query(*q, 0, 11)                                              # without itself: the revisited keyframe first
        assert e[0] == 2 and s[0] > s[1]
    finally:
        db.close()
