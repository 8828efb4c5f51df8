"""The layout of a window's keypoint and pose-graph terms on the CPU (sage_slam_amd/csrc/window_plan.h: term_layout -- which
entry of which group's result buffers and of the {error, inliers} array a term gets, the two launch orders, the counts),
compiled on its own with the host C++ compiler as tests/test_solver_rows.py does and compared with a restatement in Python;
and the sizes TermResults (csrc/term_results.h) answers per group against the factors' own (kp_kind_dim, kGraphD)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage_slam_amd", "csrc")
KP_KINDS, GROUPS, POSE_SCALE = 3, 3, 2

DRIVER = r"""
#include "window_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
using namespace sage::plan;
static void put(const std::vector<TermSlot> &v)
{
  for (const TermSlot &s : v)
    std::printf(" %d,%d,%d,%d", s.local, s.group, s.out, s.stat);
  std::printf(" |");
}
static void put(const std::vector<int> &v)
{
  for (int x : v)
    std::printf(" %d", x);
  std::printf(" |");
}
int main()
{
  std::string line;
  while (std::getline(std::cin, line)) // family kind owned ... (family k / g) -> kp | graph | kp_order | graph_order | counts, sizes
  {
    std::istringstream in(line);
    std::string fam;
    int kind, owned;
    std::vector<TermKey> kp, graph;
    while (in >> fam >> kind >> owned)
      (fam == "k" ? kp : graph).push_back(TermKey{kind, owned != 0});
    const TermLayout L = term_layout(kp, graph);
    put(L.kp);
    put(L.graph);
    put(L.kp_order);
    put(L.graph_order);
    std::printf(" %d %d %d %d %d %d %d\n", L.count[0], L.count[1], L.count[2], L.n_keypoint(), L.n_graph(), L.n_stats(),
                L.n_photo_stats());
  }
  return 0;
}
"""

DIMS = r"""
#include "term_results.h"
#include "keypoint_batch.h"
#include "graph_terms.h"
#include <cstdio>
using namespace sage;
static_assert(TermResults::dim(plan::keypoint_kind_group(0), 32) == kp_kind_dim(0, 32), "usable in constant expressions");
int main()
{
  float a[3], b[3];
  const TermResults r{a + 0, b + 0, a + 1, b + 1, a + 2, b + 2, nullptr, 5, 6, 7};
  for (int g = 0; g < plan::kTermGroups; ++g)
    if (r.AtA(g) != a + g || r.Atb(g) != b + g)
      return 1;
  if (r.n_photo_stats() != 5 || r.n_geo_stats() != 13)
    return 2;
  for (int CS : {16, 32})
  {
    for (int kind = 0; kind < kKpKinds; ++kind)
      std::printf("%d %d ", TermResults::dim(plan::keypoint_kind_group(kind), CS), kp_kind_dim(kind, CS));
    for (int kind = 0; kind < 3; ++kind)
      std::printf("%d %d ", TermResults::dim(plan::graph_kind_group(kind), CS), kGraphD);
    for (int g = 0; g < plan::kTermGroups; ++g)
      std::printf("%d %d ", plan::term_adj_type(g), adj_group(plan::term_adj_type(g)));
    std::printf("%d %d\n", adj_group(0), adj_group(1));
  }
  return 0;
}
"""


def host_compiler():
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    return cxx


@pytest.fixture(scope="module")
def term_layout(tmp_path_factory):
    """term_layout(kp, graph), each a list of (kind, owned) in add order -> the compiled header's answer as a dict"""
    d = tmp_path_factory.mktemp("term_layout")
    src, exe = d / "layout_driver.cpp", d / "layout_driver"
    src.write_text(DRIVER)
    r = subprocess.run([host_compiler(), "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(kp, graph):
        words = [f"k {k} {int(o)}" for k, o in kp] + [f"g {k} {int(o)}" for k, o in graph]
        out = subprocess.run([str(exe)], input=" ".join(words) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        parts = out.stdout.strip().split("|")
        slots = lambda s: [tuple(int(x) for x in w.split(",")) for w in s.split()]
        ints = lambda s: [int(x) for x in s.split()]
        tail = ints(parts[4])
        return dict(kp=slots(parts[0]), graph=slots(parts[1]), kp_order=ints(parts[2]), graph_order=ints(parts[3]),
                    count=tail[:3], n_keypoint=tail[3], n_graph=tail[4], n_stats=tail[5], n_photo_stats=tail[6])
    return ask


def restated(kp, graph):
    """the rule in ten lines: keypoint terms kind-major in add order, then the graph terms in add order -- that position is
    `stat`; `out` counts within the group (keypoint kind = group, every graph kind = the pose-scale group); within a family the
    position is `local`"""
    kp_order = [i for kind in range(KP_KINDS) for i, (k, own) in enumerate(kp) if k == kind and own]
    graph_order = [i for i, (_k, own) in enumerate(graph) if own]
    count, stat = [0] * GROUPS, 0
    kp_slots, graph_slots = [(-1, -1, -1, -1)] * len(kp), [(-1, -1, -1, -1)] * len(graph)
    for slots, order in ((kp_slots, kp_order), (graph_slots, graph_order)):
        for local, i in enumerate(order):
            g = kp[i][0] if slots is kp_slots else POSE_SCALE
            slots[i] = (local, g, count[g], stat)
            count[g] += 1
            stat += 1
    return dict(kp=kp_slots, graph=graph_slots, kp_order=kp_order, graph_order=graph_order, count=count,
                n_keypoint=len(kp_order), n_graph=len(graph_order), n_stats=len(kp_order) + len(graph_order),
                n_photo_stats=sum(1 for k, own in kp if k == 0 and own))


ALL_SIX = ([(2, 1), (0, 1), (1, 0), (1, 1), (0, 0), (2, 1), (0, 1), (1, 1), (2, 0), (0, 1)],         # keypoint kinds, interleaved
           [(1, 1), (0, 1), (2, 0), (2, 1), (0, 0), (1, 1), (0, 1)])                                 # graph kinds
CASES = {
    "no terms": ([], []),
    "graph terms only": ([], [(0, 1), (2, 1), (1, 1), (0, 1)]),
    "keypoint terms only": ([(1, 1), (0, 1), (2, 1), (0, 1), (1, 1)], []),
    "all six kinds interleaved, some not owned": ALL_SIX,
    "everything not owned": tuple([(k, 0) for k, _ in fam] for fam in ALL_SIX),
}


@pytest.mark.parametrize("name", list(CASES))
def test_term_layout_matches_its_restatement(term_layout, name):
    kp, graph = CASES[name]
    got, ref = term_layout(kp, graph), restated(kp, graph)
    assert got == ref
    n_loop_mg = sum(1 for k, own in kp if k == 2 and own)
    for fam, slots, order in ((kp, got["kp"], got["kp_order"]), (graph, got["graph"], got["graph_order"])):
        owned = [i for i, (_k, own) in enumerate(fam) if own]
        # local indices: a permutation of 0 .. n_local - 1, -1 exactly for the terms of another rank; the launch order is its inverse
        assert sorted(s[0] for i, s in enumerate(slots) if i in owned) == list(range(len(owned)))
        assert all(s == (-1, -1, -1, -1) for i, s in enumerate(slots) if i not in owned)
        assert [slots[i][0] for i in order] == list(range(len(order))) and sorted(order) == owned
    # `out`: dense within each group, add order within a kind, graph terms from the loop-MG count on
    for g in range(GROUPS):
        outs = sorted(s[2] for s in got["kp"] + got["graph"] if s[1] == g)
        assert outs == list(range(got["count"][g]))
    for kind in range(KP_KINDS):
        mine = [got["kp"][i] for i, (k, own) in enumerate(kp) if k == kind and own]
        assert [s[2] for s in mine] == list(range(len(mine))) and all(s[1] == kind for s in mine)
    gs = [got["graph"][i] for i in got["graph_order"]]
    assert [s[2] for s in gs] == list(range(n_loop_mg, n_loop_mg + len(gs))) and all(s[1] == POSE_SCALE for s in gs)
    # `stat`: the kind-major keypoint order, then the graph terms
    assert [got["kp"][i][3] for i in got["kp_order"]] == list(range(got["n_keypoint"]))
    assert [s[3] for s in gs] == list(range(got["n_keypoint"], got["n_stats"]))
    kinds_in_stat_order = [kp[i][0] for i in got["kp_order"]]
    assert kinds_in_stat_order == sorted(kinds_in_stat_order)
    # counts and the photometric share: the leading `stat` entries are the reprojection terms
    assert got["n_photo_stats"] == kinds_in_stat_order.count(0) == got["count"][0]
    assert got["count"] == [kinds_in_stat_order.count(0), kinds_in_stat_order.count(1), n_loop_mg + len(gs)]
    assert got["n_stats"] == sum(got["count"])


def test_group_sizes_are_the_factors_own(tmp_path):
    """TermResults' accessors compiled on the host: dim(group, CS) against kp_kind_dim and kGraphD at CS 16 and 32, the
    select chains, and the adjacency type of a group back to the group"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.isdir(os.path.join(rocm, "include", "hip")):
        pytest.skip("no HIP headers installed")
    src, exe = tmp_path / "dims.cpp", tmp_path / "dims"
    src.write_text(DIMS)
    r = subprocess.run([host_compiler(), "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr)
    lines = [[int(x) for x in l.split()] for l in out.stdout.strip().splitlines()]
    assert len(lines) == 2
    for CS, v in zip((16, 32), lines):
        pairs = list(zip(v[0:12:2], v[1:12:2]))
        assert all(a == b for a, b in pairs), (CS, pairs)
        assert [a for a, _ in pairs] == [13 + CS, 14 + 2 * CS, 14, 14, 14, 14]
        assert v[12:18] == [2, 0, 3, 1, 4, 2] and v[18:] == [0, 1]
