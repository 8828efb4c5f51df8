"""sage_vocabulary_build (DBoW2's hierarchical k-means on the device) against the numpy restatement tests/voc_build_ref.py.

Cases (tests/test_voc_build_ref.py::CASES): the generic path (k = 3, L = 2, C = 5, M = 40 in 4 documents); one root node of
M = 255, 256, 257 and 513 points whose seeding picks the last point (the tile edges of the assignment and of the seeding's
scan, the cut in the last tile, an empty document); a child of n <= k points and a child of one point; a node of identical
points (dist_sum = 0: one child); every point twice (min_d = 0 entries); a cluster emptied in a later round (it keeps its
centre and becomes a leaf no point is on); k = 64, C = 64 (the LDS maximum), M = 4096; the shipped shape k = 10, L = 3,
C = 16 on planted data, M = 20 000 in 20 documents; max_iterations = 2.
Also: TF / IDF / BINARY weights, the written file read back, and the document counts taken one document per pass.

Bound: none on the decisions.  tests/test_voc_build_ref.py::test_gpu_cases_are_decidable shows that in every case no point
has two centres within 4 (C + 2) 2^-24 of each other in any round, no seeding cut lies that close to a running sum and no
mean lies within the fp64 summation error of an fp32 rounding boundary: the tree, the word ids, the document counts, the
node of EVERY point and the rounds per level are compared for equality (leave-out cap: zero), descriptors to 1 fp32 ulp,
weights to 4 * 2^-53 relative (libm's log against numpy's).

Measured on an MI355X: every case equal -- 0 descriptor values off by one ulp in any case (6 ... 17 776 values), nodes / words
5 / 4 (tiles) ... 1 111 / 1 000 (shipped), Lloyd rounds per level [2] ... [14] (tile257), [4, 4, 6] for the shipped shape with
30 / 30 / 34 launches and 5 / 5 / 7 waits, 134 launches at k = 64 (63 seeding rounds), 3 nodes capped by max_iterations = 2; the
whole file runs in about 3 s."""
import numpy as np
import pytest

from tests.test_voc_build_ref import CASES, case

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


def dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(capi, ws, c):
    b = capi.VocabularyBuild(ws, dev(c["desc"]), c["doc_begin"], k=c["k"], L=c["L"], seed=c["seed"], weighting=c["weighting"],
                             max_iterations=c["max_iterations"])
    out = dict(voc=b.voc, ni=b.docs_with_word, node=b.node_of_point().cpu().numpy(), stats=b.stats)
    b.close()
    return out


def raw(o):
    v = o["voc"]
    return b"".join(v[key].tobytes() for key in ("parent", "descriptors", "weight", "word_id")) + o["ni"].tobytes() + \
        o["node"].tobytes() + bytes(memoryview(o["stats"]))


def ulps(a, b):
    """distance in fp32 ulps of two float32 arrays of finite values"""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(np.ascontiguousarray(a, np.float32)) - key(np.ascontiguousarray(b, np.float32)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_equals_the_restatement(capi, ws, name):
    c = case(name)
    r = c["ref"]
    o = run(capi, ws, c)
    v, st = o["voc"], o["stats"]
    L, k = c["L"], c["k"]
    print(name, "nodes", v["n_nodes"], "words", v["n_words"], "rounds", list(st.rounds)[:L], "launches", list(st.launches)[:L],
          "waits", list(st.waits)[:L], "capped", st.nodes_capped)
    assert np.array_equal(v["parent"], r["parent"])
    assert np.array_equal(v["word_id"], r["word_id"])
    assert (st.n_nodes, st.n_words, st.levels, st.nodes_capped) == (r["n_nodes"], r["n_words"], r["levels"], r["nodes_capped"])
    assert list(st.nodes)[:L] == r["nodes"] and list(st.kmeans_nodes)[:L] == r["kmeans_nodes"]
    assert list(st.rounds)[:L] == r["rounds"]
    assert np.array_equal(o["node"], r["node_of_point"])
    assert np.array_equal(o["ni"], r["docs_with_word"])
    d = ulps(v["descriptors"], r["descriptors"])
    print(name, "descriptor values off by one ulp:", int((d == 1).sum()), "of", d.size)
    assert int(d.max()) <= 1
    w, wr = v["weight"], r["weight"]
    assert np.array_equal(w == 0, wr == 0) and np.all(np.abs(w - wr) <= 4 * 2.0 ** -53 * np.abs(wr))
    # the launches of a round are the plan's, whatever the number of nodes
    rc, plan = capi.vocabulary_build_plan_raw(c["desc"].shape[0], c["desc"].shape[1], k, L)
    assert rc == 0
    for l in range(st.levels):
        seed_rounds = k - 1 if r["kmeans_nodes"][l] else 0
        assert st.seed_rounds[l] == seed_rounds and st.waits[l] == st.rounds[l] + 1
        assert st.launches[l] == 1 + plan["launches_per_seed_round"] * seed_rounds + plan["launches_per_lloyd_round"] * st.rounds[l] + \
            (3 if r["kmeans_nodes"][l] else 2)
    # two builds give identical bytes
    assert raw(run(capi, ws, c)) == raw(o)
    # sage_vocabulary_create accepts the result, and the walk sends every training point to the word of the node the build
    # reports for it: the trainer tied to the walk with no restatement in between (duplicates inside a node of n <= k points
    # aside: no case has any)
    voc = capi.Vocabulary(v)
    assert (voc.num_nodes, voc.num_words, voc.channels) == (v["n_nodes"], v["n_words"], v["C"])
    ids, vals, bs, words = capi.bow_transform(ws, voc, dev(c["desc"]), per_point=True)
    voc.close()
    assert np.array_equal(words.cpu().numpy(), v["word_id"][o["node"]])
    assert bs.n_leaves_hit == int(np.unique(o["node"]).size)


def test_other_weightings_and_the_file(capi, ws, tmp_path):
    """TF / BINARY: every word 1 and no document counts; IDF as TF_IDF; the result written and read back is the result."""
    from sage_slam_amd import vocabulary
    c = case("generic")
    base = run(capi, ws, c)
    for weighting in (1, 3):
        o = run(capi, ws, dict(c, weighting=weighting))
        leaves = o["voc"]["word_id"] >= 0
        assert np.all(o["voc"]["weight"][leaves] == 1.0) and np.all(o["voc"]["weight"][~leaves] == 0.0) and not o["ni"].any()
        assert np.array_equal(o["voc"]["descriptors"], base["voc"]["descriptors"]) and o["voc"]["weighting"] == weighting
    o = run(capi, ws, dict(c, weighting=2))
    assert np.array_equal(o["voc"]["weight"], base["voc"]["weight"]) and np.array_equal(o["ni"], base["ni"])
    p = str(tmp_path / "built.yml.gz")
    vocabulary.save_opencv_yaml(base["voc"], p)
    back = vocabulary.load_opencv_yaml(p)
    for key in ("parent", "descriptors", "weight", "word_id"):
        assert back[key].tobytes() == base["voc"][key].tobytes(), key
    assert (back["k"], back["L"], back["weighting"], back["scoring"]) == (c["k"], c["L"], 0, 0)


@pytest.mark.parametrize("name", ["generic", "tile257"])
def test_document_counts_in_chunks(capi, ws, monkeypatch, name):
    """The document counts take the documents in chunks that fit the flag buffer; with a budget of one byte a chunk is one
    document (four passes; tile257 has an empty document): the same Ni, the same weights, the same bytes."""
    c = case(name)
    whole = run(capi, ws, c)
    monkeypatch.setenv("SAGE_VOC_FLAG_BYTES", "1")
    chunked = run(capi, ws, c)
    assert np.array_equal(chunked["ni"], c["ref"]["docs_with_word"]) and raw(chunked) == raw(whole)
