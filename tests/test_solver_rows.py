"""Solver rows on the CPU: the rule that decides which groups of a keyframe's block a window solves for
(sage_slam_amd/csrc/window_plan.h: solver_rows -- a group every keyframe holds is left out), compiled on its own with the host
C++ compiler as tests/test_window_plan.py does, and the host block solver at the block sizes such windows bring (B = 6, 7, 8:
blocks padded to 8 rows) against numpy.linalg.solve at the bar of tests/test_host_logic.py (1e-9)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sage_slam_amd import capi
from tests.helpers import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage_slam_amd", "csrc")
POSE, CODE, SCALE, ALL = 1, 2, 4, 7
NOT_PSD = -3                                                     # SAGE_E_NOT_PSD

DRIVER = r"""
#include "window_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
int main()
{
  std::string line;
  while (std::getline(std::cin, line)) // CS masks... -> B Bs kept | to_block | to_solver
  {
    std::istringstream in(line);
    int CS, m;
    std::vector<unsigned char> hold;
    in >> CS;
    while (in >> m)
      hold.push_back((unsigned char)m);
    const sage::plan::SolverRows s = sage::plan::solver_rows(hold.data(), (int)hold.size(), CS);
    std::printf("%d %d %d %d |", s.B, s.Bs, s.kept, (int)s.compact());
    for (int x : s.to_block)
      std::printf(" %d", x);
    std::printf(" |");
    for (int x : s.to_solver)
      std::printf(" %d", x);
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def solver_rows(tmp_path_factory):
    """solver_rows(CS, masks) -> dict(B, Bs, kept, compact, to_block, to_solver) as the compiled header answers"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    d = tmp_path_factory.mktemp("solver_rows")
    src, exe = d / "rows_driver.cpp", d / "rows_driver"
    src.write_text(DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr

    def ask(CS, masks):
        out = subprocess.run([str(exe)], input=" ".join(str(v) for v in [CS] + list(masks)) + "\n", capture_output=True,
                             text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        head, tb, ts = ([int(x) for x in part.split()] for part in out.stdout.strip().split("|"))
        return dict(B=head[0], Bs=head[1], kept=head[2], compact=bool(head[3]), to_block=tb, to_solver=ts)
    return ask


def group_rows(CS, groups):
    rows = {POSE: list(range(6)), CODE: list(range(6, 6 + CS)), SCALE: [6 + CS]}
    return [r for grp in (POSE, CODE, SCALE) if groups & grp for r in rows[grp]]


def check_maps(s, CS, kept):
    """the answer keeps exactly the groups `kept`, in block order, and its two maps are inverse to each other"""
    B = 7 + CS
    assert s["B"] == B and s["kept"] == kept
    assert s["to_block"] == group_rows(CS, kept) and s["Bs"] == len(s["to_block"]) and len(s["to_solver"]) == B
    assert s["compact"] == (s["Bs"] != B)
    for srow, r in enumerate(s["to_block"]):
        assert s["to_solver"][r] == srow
    for r, srow in enumerate(s["to_solver"]):
        assert srow == -1 if r not in s["to_block"] else s["to_block"][srow] == r


@pytest.mark.parametrize("CS", [32, 16, 1])
@pytest.mark.parametrize("K", [1, 6])
def test_a_group_is_dropped_exactly_when_every_keyframe_holds_it(solver_rows, CS, K):
    B = 7 + CS
    nothing = solver_rows(CS, [0] * K)
    check_maps(nothing, CS, ALL)
    assert nothing["Bs"] == B and not nothing["compact"] and nothing["to_block"] == list(range(B))
    # the table of sage_window_hold: codes; codes and scales; poses
    for all_hold, kept, Bs in ((CODE, POSE | SCALE, 7), (CODE | SCALE, POSE, 6), (POSE, CODE | SCALE, 1 + CS)):
        s = solver_rows(CS, [all_hold] * K)
        check_maps(s, CS, kept)
        assert s["Bs"] == Bs
        # holds beyond the common ones (the loop graph: keyframe 0 holds everything) stay inside the kept groups
        if K > 1:
            more = solver_rows(CS, [ALL] + [all_hold] * (K - 1))
            assert more == s
    everything = solver_rows(CS, [ALL] * K)
    check_maps(everything, CS, ALL)                              # nothing left to solve for: the window solves at B
    assert everything["Bs"] == B and not everything["compact"]


def test_one_free_keyframe_keeps_the_group(solver_rows):
    CS, K = 32, 6
    for free in range(K):
        masks = [CODE] * K
        masks[free] = 0
        s = solver_rows(CS, masks)
        check_maps(s, CS, ALL)
        assert s["Bs"] == 7 + CS
    masks = [CODE | SCALE] * K
    masks[3] = CODE                                              # one free scale: the scales stay, the codes go
    s = solver_rows(CS, masks)
    check_maps(s, CS, POSE | SCALE)
    assert s["Bs"] == 7
    assert solver_rows(CS, [])["Bs"] == 7 + CS                   # no keyframes: nothing held by all


# ------------------------------------------------------------------------------------------- the host solver at B = 6, 7, 8
def dense_window_system(K, B, links, seed, shift):
    """an SPD system with the packed sparsity of `links` -> (packed with a zero tail, H, g)"""
    rng = np.random.default_rng(seed)
    n = K * B
    mask = np.eye(K, dtype=bool)
    for a, b in links:
        mask[a, b] = mask[b, a] = True
    J = rng.normal(size=(3 * n, n))
    Hs = (J.T @ J) * np.kron(mask, np.ones((B, B))) + shift * n * np.eye(n)
    g = rng.normal(size=n)
    diag = np.stack([Hs[k * B:(k + 1) * B, k * B:(k + 1) * B] for k in range(K)])
    lnk = np.stack([Hs[a * B:(a + 1) * B, b * B:(b + 1) * B] for a, b in links])
    return np.concatenate([diag.reshape(-1), lnk.reshape(-1), g, np.zeros(4)]), Hs, g


@pytest.mark.parametrize("B", [6, 7, 8, 1])
def test_block_solve_at_eight_row_blocks_matches_dense(B):
    """the band + loop-closure graph of test_block_solve_matches_dense at the block sizes padded to 8 rows"""
    K = 7
    links = [(j, i) for i in range(K) for j in range(max(0, i - 3), i)] + [(0, 6)]
    packed, Hs, g = dense_window_system(K, B, links, seed=3 + B, shift=5)
    rng = np.random.default_rng(B)
    n = K * B
    dadd = rng.uniform(0, 1, n); gadd = rng.normal(size=n)
    d = capi.block_solve(packed, K, links, B, 1e-3, dadd, gadd)
    Hf = Hs + np.diag(dadd)
    ref = np.linalg.solve(Hf + 1e-3 * np.diag(np.diag(Hf)), g + gadd)
    assert rel(d, ref) < 1e-9
    with pytest.raises(capi.SageError) as ei:                           # not positive definite
        capi.block_solve(-packed, K, links, B, 0.0)
    assert ei.value.code == NOT_PSD


@pytest.mark.parametrize("K,window", [(24, 3), (20, 5), (33, 1)])
def test_block_solve_split_window_at_pose_scale_blocks_matches_dense(K, window, monkeypatch):
    """the family of test_block_solve_split_window_matches_dense at B = 7: two halves and a separator, split or not, helper
    claimed or not; a loop closure changes the plan"""
    B = 7
    for extra in ([], [(1, K - 2)]):
        links = [(j, i) for i in range(K) for j in range(max(0, i - window), i)] + extra
        packed, Hs, g = dense_window_system(K, B, links, seed=K, shift=6)
        ref = np.linalg.solve(Hs + 1e-4 * np.diag(np.diag(Hs)), g)
        out = []
        for no_split in (None, "1"):
            if no_split:
                monkeypatch.setenv("SAGE_SOLVE_NO_SPLIT", no_split)
            else:
                monkeypatch.delenv("SAGE_SOLVE_NO_SPLIT", raising=False)
            for _ in range(3):                                          # repeated: helper claimed / not claimed
                d = capi.block_solve(packed, K, links, B, 1e-4)
                assert rel(d, ref) < 1e-9
                out.append(d)
        assert rel(out[0], out[-1]) < 1e-11


def test_block_solve_ring_closure_at_pose_scale_blocks_matches_dense():
    """a long ring with chords (the shape of the loop-closure graph: arrow rows, the worker pool) at B = 7"""
    K, B = 96, 7
    links = sorted({(min(k, (k + s) % K), max(k, (k + s) % K)) for k in range(K) for s in (1, 2)})
    packed, Hs, g = dense_window_system(K, B, links, seed=96, shift=6)
    ref = np.linalg.solve(Hs + 1e-3 * np.diag(np.diag(Hs)), g)
    for _ in range(3):
        assert rel(capi.block_solve(packed, K, links, B, 1e-3), ref) < 1e-9


@pytest.mark.parametrize("K,loops", [(64, []), (40, [(0, 39), (3, 30)]), (30, [(2, 27)])])
@pytest.mark.parametrize("ndomains", [1, 2, 4])
def test_block_solve_domains_at_pose_scale_blocks_equals_block_solve(K, loops, ndomains):
    """sage_block_solve_domains (the sharded solve's partial factorisation and Schur rows) at B = 7, as
    tests/test_shard_schur.py runs it at the larger blocks"""
    B = 7
    links = [(j, i) for i in range(K) for j in range(max(0, i - 3), i)] + loops
    packed, Hs, g = dense_window_system(K, B, links, seed=3 * K + ndomains, shift=6)
    rng = np.random.default_rng(2)
    dadd = np.full(K * B, 1e-3); gadd = 1e-3 * rng.normal(size=K * B)
    dadd[:6] += 1e4
    ref = capi.block_solve(packed[:-4], K, links, B, 1e-3, dadd, gadd)
    Hf = Hs + np.diag(dadd)
    assert rel(ref, np.linalg.solve(Hf + 1e-3 * np.diag(np.diag(Hf)), g + gadd)) < 1e-9
    d = capi.block_solve_domains(packed, K, links, B, 1e-3, ndomains, dadd, gadd)
    assert rel(d, ref) < 1e-9


def test_the_solver_block_size_is_declared_and_bound():
    L = capi.lib()
    assert "sage_window_solver_block_size" in capi.SYMBOLS and hasattr(L, "sage_window_solver_block_size")
    assert L.sage_window_solver_block_size(None) == 0 and L.sage_window_block_size(None) == 0
