"""The window engine's build-time policy (sage_slam_amd/csrc/window_plan.h) on the CPU: edge ownership against its Python mirror
(capi.shard_edges / capi.shard_links), the run-length rules against a table evaluated from the rules as they stood inside
sage_window_finalize, the tuning candidates.  The header is compiled on its own with the host C++ compiler: that it needs nothing
but the standard library is one of the assertions."""
import os
import re
import shutil
import subprocess

import pytest

from sage_slam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage_slam_amd", "csrc")

DRIVER = r"""
#include "window_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
using namespace sage::plan;
static void put(const std::vector<int> &v)
{
  for (int x : v)
    std::printf(" %d", x);
}
int main()
{
  std::string line;
  while (std::getline(std::cin, line))
  {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "own") // nlinks rank world by_link -> edges | links
    {
      int n, r, w, bl;
      in >> n >> r >> w >> bl;
      const Ownership o = owned_edges(n, r, w, bl != 0);
      put(o.edges);
      std::printf(" |");
      put(o.links);
    }
    else if (cmd == "run") // FS tiles... -> geometric run, photometric run, record cadence, runs of the typical edge
    {
      int FS, t;
      std::vector<int> tiles;
      in >> FS;
      while (in >> t)
        tiles.push_back(t);
      const int p = photo_run(tiles, FS);
      std::printf(" %d %d %d %d", geo_run(total_tiles(tiles)), p, record_cadence(p), (typical_edge(tiles) + p - 1) / p);
    }
    else if (cmd == "cand") // rule typical -> candidates
    {
      int rule, typical;
      in >> rule >> typical;
      put(tune_candidates(rule, typical));
    }
    else if (cmd == "schur") // world K requested -> 0 / 1
    {
      int w, K, req;
      in >> w >> K >> req;
      std::printf(" %d", (int)uses_domain_solve(w, K, req));
    }
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(queries) -> per query line the integers the compiled header answers (ownership: [edges, links])"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    d = tmp_path_factory.mktemp("window_plan")
    src, exe = d / "plan_driver.cpp", d / "plan_driver"
    src.write_text(DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr

    def ask(queries):
        out = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = out.stdout.split("\n")[:-1]
        assert len(rows) == len(queries)
        ints = lambda s: [int(x) for x in s.split()]
        return [[ints(part) for part in row.split("|")] if "|" in row else ints(row) for row in rows]
    return ask


def test_header_names_no_device_runtime_and_no_environment():
    text = open(os.path.join(CSRC, "window_plan.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", text, re.M)
    assert includes and all(re.fullmatch(r"<[a-z_]+>", i) for i in includes), includes
    assert "getenv" not in text and not re.search(r"\bhip[A-Za-z_]", text)


def test_ownership_matches_the_python_mirror_and_partitions_the_edges(plan):
    cases = [(n, w) for n in list(range(41)) + [186, 372, 1530] for w in range(1, 9)]
    answers = iter(plan([f"own {n} {r} {w} {bl}" for n, w in cases for r in range(w) for bl in (0, 1)]))
    for n, w in cases:
        seen = {0: [], 1: []}
        for r in range(w):
            for bl in (0, 1):
                edges, links = next(answers)
                if bl == 0:
                    assert edges == capi.shard_edges(n, r, w), (n, r, w)
                else:
                    assert edges == [e for l in capi.shard_links(n, r, w) for e in (2 * l, 2 * l + 1)], (n, r, w)
                assert links == sorted(set(e // 2 for e in edges)), (n, r, w, bl)
                seen[bl] += edges
        for bl in (0, 1):   # the ranks' lists one after the other: disjoint, ascending, every directed edge
            assert seen[bl] == list(range(2 * n)), (n, w, bl)


# (sub-tiles per edge, FS) -> geometric run, photometric run, record cadence (0: one record per workgroup), runs of the typical
# edge.  Expected values: the rules of sage_window_finalize as they stood before they moved into the header, evaluated by hand,
# no environment overrides; None: not part of the row
RUNS = [
    ([80] * 372, 16, 16, 10, 5, 8),      # headline window, 128 x 160
    ([63] * 372, 16, 16, 8, 4, 8),       # "63 sub-tiles = 8 runs of 8"
    ([252] * 84, 32, 16, 8, 4, 32),      # BASELINE config 4: 32 runs
    ([252] * 11, 32, 4, 8, 4, 32),       # config 4, one rank of 8: the FS = 32 band's 6, overridden by the multiple-of-8 pick
    ([252] * 10, 32, 4, 8, 4, 32),
    ([63] * 47, 16, 4, 4, 0, 16),        # K = 64, one rank of 8
    ([12] * 3000, 16, 16, 6, 3, 2),      # 3072 samples per keyframe: T = 12 -> runs of 6
    ([165] * 84, 16, 16, 6, 3, 28),      # 192 x 256: runs of 6 = 28 per edge
    ([50] * 40, 16, 4, 15, 5, 4),
    ([320] * 84, 32, 16, 8, 4, 40),
    ([20] * 6, 16, 2, 1, 0, 20),
    ([1] * 2, 16, 2, 1, 0, 1),
    ([63, 63, 63, 10, 10, 80, 80], 16, None, 8, 4, None),
]


def test_run_lengths(plan):
    answers = plan(["run %d %s" % (fs, " ".join(map(str, tiles))) for tiles, fs, *_ in RUNS])
    for (tiles, fs, *want), got in zip(RUNS, answers):
        assert [g if x is not None else None for g, x in zip(got, want)] == want, (len(tiles), tiles[0], fs, got)


def test_tuning_candidates(plan):
    assert plan(["cand 8 63", "cand 10 80", "cand 4 5"]) == [[8, 4, 6, 9, 10, 12, 16], [10, 4, 6, 8, 9, 12, 16], [4]]


def test_domain_solve_predicate(plan):
    # sharded windows only; a request (0 / 1) wins over the K >= 256 default
    queries = ["schur 1 512 -1", "schur 1 64 1", "schur 8 64 -1", "schur 8 255 -1", "schur 8 256 -1", "schur 8 64 1",
               "schur 8 512 0", "schur 2 256 -1"]
    assert [a[0] for a in plan(queries)] == [0, 0, 0, 0, 1, 1, 0, 1]
