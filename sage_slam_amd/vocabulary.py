"""Reading and writing the loop detector's vocabulary file: the OpenCV FileStorage YAML (``%YAML:1.0``, optionally gzipped) that
``TemplatedTensorVocabulary::load`` (``core/system/tensor_vocabulary.cpp:49-128``) reads and DBoW2's ``save`` writes.

The file is flat enough for ``gzip`` + ``re``: a header (k, L, scoringType, weightingType), one flow mapping per node
(nodeId, parentId, weight, descriptor: C floats in a string) and one per word (wordId, nodeId).  No OpenCV is needed.
"""
from __future__ import annotations

import gzip
import re

import numpy as np

_HEADER = {name: re.compile(r"^\s*" + name + r":\s*(-?\d+)\s*$", re.M) for name in ("k", "L", "scoringType", "weightingType")}
_NODE = re.compile(r"\{\s*nodeId:\s*(\d+)\s*,\s*parentId:\s*(\d+)\s*,\s*weight:\s*([^,\s]+)\s*,\s*descriptor:\s*\"([^\"]*)\"\s*\}")
_WORD = re.compile(r"\{\s*wordId:\s*(\d+)\s*,\s*nodeId:\s*(\d+)\s*\}")
SCORING_NAMES = ("L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT")   # DBoW2::ScoringType
WEIGHTING_NAMES = ("TF_IDF", "TF", "IDF", "BINARY")                                          # DBoW2::WeightingType


def load_opencv_yaml(path: str) -> dict:
    """-> dict(parent [n] int32 (parent[0] = -1), descriptors [n, C] float32 (row 0, the root's, is zero), weight [n]
    float64, word_id [n] int32 (-1 for an inner node), k, L, scoring, weighting (DBoW2's enum values), n_nodes, n_words, C):
    the arrays ``sage_vocabulary_create`` takes; index = the file's nodeId.

    Raises ValueError when the file is not such a vocabulary, and when the children of a node are not listed in ascending
    nodeId: the reference orders a node's children as the file lists them (and its argmin lets the first smallest win), the
    library by ascending node index -- the two must be the same order."""
    with open(path, "rb") as fh:
        raw = fh.read()
    text = (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode("ascii")
    if not text.startswith("%YAML:1.0") or "vocabulary:" not in text:
        raise ValueError(f"{path}: not an OpenCV %YAML:1.0 vocabulary file")
    head = {}
    for name, rx in _HEADER.items():
        m = rx.search(text)
        if not m:
            raise ValueError(f"{path}: no '{name}' entry")
        head[name] = int(m.group(1))
    at_words = text.find("\n   words:")
    if at_words < 0:
        at_words = text.find("words:")
    nodes = _NODE.findall(text[:at_words] if at_words >= 0 else text)
    words = _WORD.findall(text[at_words:]) if at_words >= 0 else []
    if not nodes or not words:
        raise ValueError(f"{path}: no nodes or no words")
    n = len(nodes) + 1
    ids = np.array([int(t[0]) for t in nodes], np.int64)
    if not np.array_equal(np.sort(ids), np.arange(1, n)):
        raise ValueError(f"{path}: the node ids are not 1..{n - 1}")
    C = len(nodes[0][3].split())
    parent = np.full(n, -1, np.int32)
    weight = np.zeros(n, np.float64)
    desc = np.zeros((n, C), np.float32)
    last_child = {}
    for nid, pid, w, d in nodes:
        nid, pid = int(nid), int(pid)
        if last_child.get(pid, 0) > nid:
            raise ValueError(f"{path}: the children of node {pid} are not listed in ascending nodeId ({last_child[pid]} before {nid})")
        last_child[pid] = nid
        vals = d.split()
        if len(vals) != C:
            raise ValueError(f"{path}: node {nid} has {len(vals)} descriptor values, node {nodes[0][0]} has {C}")
        parent[nid] = pid
        weight[nid] = float(w)
        desc[nid] = np.array([float(v) for v in vals], np.float64).astype(np.float32)
    word_id = np.full(n, -1, np.int32)
    for wid, nid in words:
        if not 0 < int(nid) < n:
            raise ValueError(f"{path}: word {wid} names node {nid}")
        word_id[int(nid)] = int(wid)
    return dict(parent=parent, descriptors=desc, weight=weight, word_id=word_id, k=head["k"], L=head["L"],
                scoring=head["scoringType"], weighting=head["weightingType"], n_nodes=n, n_words=len(words), C=C)


def _yaml_double(v: float) -> str:
    """a double the way OpenCV's FileStorage writes it: integers as ``1.``, everything else with 17 significant digits"""
    v = float(v)
    if v == int(v) and abs(v) < 1e15:
        return f"{int(v)}."
    return f"{v:.16e}"


def save_opencv_yaml(voc: dict, path: str, digits: int = 9) -> None:
    """Write ``voc`` (the dict ``load_opencv_yaml`` returns, ``synth.make_vocabulary`` makes and ``capi.VocabularyBuild.voc``
    holds) as the file DBoW2's ``save`` (``TemplatedVocabulary.h:1354-1447``) writes and both ``load_opencv_yaml`` and the
    reference's ``load`` read: the header keys; the nodes in the order ``save`` lists them -- the children of the node on top
    of its parents stack in child order, every child that has children pushed in turn, so the LAST such child comes next --;
    the words in word order; gzip when ``path`` ends in ``.gz``.
    ``digits``: significant digits of a descriptor value; 9 reproduces every float32 bit, 6 is the precision of
    ``FTensor::toString`` (an ostream's default).  Weights are written with 17 significant digits.
    Raises ValueError unless a node's children ascend with the node index (they always do: children are listed by index)
    and the word ids are a permutation on the leaves."""
    parent = np.asarray(voc["parent"], np.int64)
    desc = np.asarray(voc["descriptors"], np.float32)
    weight = np.asarray(voc["weight"], np.float64)
    word_id = np.asarray(voc["word_id"], np.int64)
    n = int(parent.shape[0])
    if n < 2 or parent[0] != -1 or np.any(parent[1:] < 0) or np.any(parent[1:] >= np.arange(1, n)):
        raise ValueError("not a vocabulary tree: parent[0] must be -1 and 0 <= parent[i] < i")
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[int(parent[i])].append(i)
    leaves = [i for i in range(1, n) if not kids[i]]
    if sorted(int(word_id[i]) for i in leaves) != list(range(len(leaves))) or np.any(word_id[[i for i in range(n) if kids[i]]] >= 0):
        raise ValueError("the word ids are not a permutation of 0..n_words-1 on the leaves")
    out = ["%YAML:1.0", "---", "vocabulary:", f"   k: {int(voc['k'])}", f"   L: {int(voc['L'])}",
           f"   scoringType: {int(voc.get('scoring', 0))}", f"   weightingType: {int(voc.get('weighting', 0))}", "   nodes:"]
    fmt = "%." + str(int(digits)) + "g"
    stack = [0]
    while stack:
        pid = stack.pop()
        for c in kids[pid]:
            text = "".join(fmt % float(v) + " " for v in desc[c])
            out.append(f"      - {{ nodeId:{c}, parentId:{pid}, weight:{_yaml_double(weight[c])},")
            out.append(f"          descriptor:\"{text}\" }}")
            if kids[c]:
                stack.append(c)
    out.append("   words:")
    node_of_word = sorted((int(word_id[i]), i) for i in leaves)
    for w, i in node_of_word:
        out.append(f"      - {{ wordId:{w}, nodeId:{i} }}")
    raw = ("\n".join(out) + "\n").encode("ascii")
    if path.endswith(".gz"):
        raw = gzip.compress(raw, mtime=0)
    with open(path, "wb") as fh:
        fh.write(raw)
