"""Reading the loop detector's vocabulary file: the OpenCV FileStorage YAML (``%YAML:1.0``, optionally gzipped) that
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
