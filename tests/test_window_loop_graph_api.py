"""Loop-closure pose-scale graphs on the window engine, the parts that need no GPU: the header and exports of
sage_window_add_keypoint_link / sage_window_hold, the ctypes mirror of the third term kind, argument checks that come before
any device call, the plan's choice of the dense edges, the loop-MG generators against the oracle, and the D = 14 column map."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sage_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage_slam_amd", "csrc")
INVALID = -1


def test_header_declares_and_library_exports_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    L = capi.lib()
    for name in ("sage_window_add_keypoint_link", "sage_window_hold"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"SAGE_KP_REPROJECTION\s*=\s*0\s*,\s*SAGE_KP_MATCH_GEOMETRY\s*=\s*1\s*,\s*SAGE_KP_LOOP_MG\s*=\s*2", hdr)
    assert re.search(r"SAGE_HOLD_POSE\s*=\s*1\s*,\s*SAGE_HOLD_CODE\s*=\s*2\s*,\s*SAGE_HOLD_SCALE\s*=\s*4", hdr)
    assert (capi.SAGE_KP_REPROJECTION, capi.SAGE_KP_MATCH_GEOMETRY, capi.SAGE_KP_LOOP_MG) == (0, 1, 2)
    assert (capi.SAGE_HOLD_POSE, capi.SAGE_HOLD_CODE, capi.SAGE_HOLD_SCALE) == (1, 2, 4)
    body = re.search(r"typedef struct SageKeypointTerm\s*\{(.*?)\}\s*SageKeypointTerm;", hdr, re.S)
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    assert fields == [f[0] for f in capi.SageKeypointTerm._fields_]
    assert fields[-2:] == ["unscaled_dpts0", "matched_unscaled_dpts1"]
    assert [capi.kp_term_dim(k, 32) for k in ("reprojection", "match_geometry", "loop_mg", 2)] == [45, 78, 14, 14]


def test_bad_calls_answer_invalid_without_a_device():
    L = capi.lib()
    assert L.sage_window_add_keypoint_link(None, 0, 1) == INVALID
    assert L.sage_window_hold(None, 0, capi.SAGE_HOLD_POSE) == INVALID
    assert L.sage_window_hold(None, 0, 8) == INVALID and L.sage_window_hold(None, 0, -1) == INVALID     # bad masks
    t = capi.SageKeypointTerm()                                  # kind 2 without its depth arrays
    t.kind, t.edge, t.N = capi.SAGE_KP_LOOP_MG, 0, 8
    t.loss_param, t.weight = 1.0, 1.0
    assert L.sage_window_add_keypoint_term(None, C.byref(t)) == INVALID


# ---------------------------------------------------------------------------------------------- window_plan.h: dense edges
DRIVER = r"""
#include "window_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
using namespace sage::plan;
int main()
{
  std::string line;
  while (std::getline(std::cin, line)) // nlinks rank world by_link flags... -> the rank's dense edges
  {
    std::istringstream in(line);
    int n, r, w, bl, f;
    in >> n >> r >> w >> bl;
    std::vector<char> dense;
    while (in >> f)
      dense.push_back((char)f);
    for (int e : dense_edges(owned_edges(n, r, w, bl != 0).edges, dense))
      std::printf(" %d", e);
    std::printf("\n");
  }
  return 0;
}
"""


def test_plan_picks_the_dense_edges_among_the_owned_ones(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    src, exe = tmp_path / "dense_driver.cpp", tmp_path / "dense_driver"
    src.write_text(DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(0)
    cases = []
    for n in (0, 1, 5, 12, 13):
        for flags in ([1] * n, [0] * n, [int(v) for v in rng.integers(0, 2, n)]):
            for world in (1, 2, 3):
                for rank in range(world):
                    for bl in (0, 1):
                        cases.append((n, rank, world, bl, flags))
    out = subprocess.run([str(exe)], input="".join(" ".join(map(str, (n, r, w, bl, *fl))) + "\n" for n, r, w, bl, fl in cases),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.split("\n")[:-1]
    assert len(rows) == len(cases)
    for (n, rank, world, bl, flags), row in zip(cases, rows):
        owned = capi.shard_edges(n, rank, world) if not bl else [e for l in capi.shard_links(n, rank, world) for e in (2 * l, 2 * l + 1)]
        assert [int(x) for x in row.split()] == [e for e in owned if flags[e // 2]], (n, rank, world, bl, flags)


# ---------------------------------------------------------------------------------------------- generators
def graph_window(K=8):
    return synth.make_window(K=K, H=48, W=64, FS=16, CS=32, L=3, n_samples=900, seed=5, loop_radius=0.08)


def test_loop_mg_generators_are_deterministic():
    w = graph_window(6)
    for make, keys in ((synth.make_loop_mg_terms_from_matches, ("loc0", "loc1", "homo0", "homo1", "u0", "u1")),
                       (synth.make_loop_mg_exact, ("loc0", "homo0", "homo1", "u0", "u1"))):
        a, b, c = make(w, 0, 1, 64, 11), make(w, 0, 1, 64, 11), make(w, 0, 1, 64, 12)
        assert a["kind"] == "loop_mg" and sorted(k for k in a if k != "kind") == sorted(keys)
        assert all(np.array_equal(a[k], b[k]) for k in keys)
        assert any(not np.array_equal(a[k], c[k]) for k in keys)
        for k in ("homo0", "homo1", "u0", "u1"):
            assert a[k].dtype == np.float32 and a[k].shape[0] == 64
        assert np.isin(a["loc0"], w.keyframes[0].loc1d).all()
    m = synth.make_match_geometry_matches(w, 2, 1, 64, 3)
    t = synth.make_loop_mg_terms_from_matches(w, 2, 1, 64, 3)
    assert all(np.array_equal(m[k], t[k]) for k in ("loc0", "loc1", "homo0", "homo1"))
    k0, k1 = w.keyframes[2], w.keyframes[1]
    assert np.array_equal(t["u0"], (k0.bias[t["loc0"]] + k0.basis[t["loc0"]] @ k0.code).astype(np.float32))
    assert np.array_equal(t["u1"], (k1.bias[t["loc1"]] + k1.basis[t["loc1"]] @ k1.code).astype(np.float32))


def test_exact_terms_have_no_residual_at_the_true_variables(orc):
    w = graph_window()
    K = len(w.keyframes)
    weight, worst = 5.0, 0.0
    for k0, k1 in [(k, (k + 1) % K) for k in range(K)] + [(k, (k + 2) % K) for k in range(K)]:
        for a, b in ((k0, k1), (k1, k0)):
            t = synth.make_loop_mg_exact(w, a, b, 64, 7)
            A, Bk = w.keyframes[a], w.keyframes[b]
            R10, t10 = synth.relative_pose(A.R_true, A.t_true, Bk.R_true, Bk.t_true)
            e = orc.match_geom_error(1, "fair", R10, t10, dpts0=t["u0"], dpts1=t["u1"], homo0=t["homo0"], homo1=t["homo1"],
                                     scale0=A.scale_true, scale1=Bk.scale_true,
                                     loss_param=float(0.1 * np.mean(np.square(A.bias, dtype=np.float64))), weight=weight)
            worst = max(worst, e)
            assert 0.0 <= e <= 1e-9 * weight, (a, b, e)
    # ... and a residual away from them (the terms do constrain the graph)
    t = synth.make_loop_mg_exact(w, 0, 1, 64, 7)
    A, Bk = w.keyframes[0], w.keyframes[1]
    R10, t10 = synth.relative_pose(A.R_true, A.t_true, Bk.R_true, Bk.t_true)
    e = orc.match_geom_error(1, "fair", R10, t10, dpts0=t["u0"], dpts1=t["u1"], homo0=t["homo0"], homo1=t["homo1"],
                             scale0=1.05 * A.scale_true, scale1=Bk.scale_true, loss_param=0.1, weight=weight)
    assert e > 1e-4


# ---------------------------------------------------------------------------------------------- column map
def test_loop_mg_results_are_assembled_into_pose_and_scale_rows_only():
    CS, K = 16, 3
    B = 7 + CS
    links = [(0, 1), (1, 2), (0, 2)]
    rng = np.random.default_rng(1)
    A = rng.normal(size=(14, 14)); A = A + A.T
    b = rng.normal(size=14)
    for role in (0, 1):
        cols = [capi.edge_col(2, role, bi, CS) for bi in range(B)]
        assert cols[:6] == [role * 6 + r for r in range(6)] and cols[6 + CS] == 12 + role
        assert cols[6:6 + CS] == [-1] * CS
    for link, d in ((2, 0), (1, 1)):
        a_, b_ = links[link]
        k0, k1 = (a_, b_) if d == 0 else (b_, a_)
        packed = capi.assemble_packed(K, links, CS, {(2, link, d): dict(AtA=A, Atb=b, error=0.25, num_inliers=7)})
        H, g, tail = capi.unpack_dense(packed, K, links, CS)
        ps = lambda k: [k * B + r for r in range(6)] + [k * B + 6 + CS]     # pose and scale rows of keyframe k
        c0, c1 = list(range(6)) + [12], list(range(6, 12)) + [13]            # ... and their columns for roles 0 / 1
        assert np.array_equal(H[np.ix_(ps(k0), ps(k0))], A[np.ix_(c0, c0)])
        assert np.array_equal(H[np.ix_(ps(k1), ps(k1))], A[np.ix_(c1, c1)])
        assert np.array_equal(H[np.ix_(ps(k0), ps(k1))], A[np.ix_(c0, c1)])
        assert np.array_equal(g[ps(k0)], b[c0]) and np.array_equal(g[ps(k1)], b[c1])
        code = [k * B + 6 + i for k in range(K) for i in range(CS)]
        assert not H[code, :].any() and not H[:, code].any() and not g[code].any()     # nothing into code rows / columns
        other = [k for k in range(K) if k not in (k0, k1)][0]
        assert not H[other * B:(other + 1) * B, :].any()
        assert tail[0] == 0 and tail[1] == 0.25                     # the geometric error slot


# ---------------------------------------------------------------------------------------------- held variables (host rule)
HOLD_DRIVER = r"""
#include "damped_system.h"
#include <cstdio>
#include <vector>
// stdin: K nlinks B CS, links, hold masks, packed, dadd, gadd -> stdout: the same three arrays after sage::hold_packed,
// then per (mask, row) of one block whether the row is held
int main()
{
  int K, nl, B, CS;
  if (std::scanf("%d %d %d %d", &K, &nl, &B, &CS) != 4)
    return 1;
  std::vector<int> links(2 * nl);
  for (int &v : links)
    if (std::scanf("%d", &v) != 1)
      return 1;
  std::vector<unsigned char> hold(K);
  for (auto &h : hold)
  {
    int v;
    if (std::scanf("%d", &v) != 1)
      return 1;
    h = (unsigned char)v;
  }
  const size_t np = (size_t)(K + nl) * B * B + (size_t)K * B;
  std::vector<double> packed(np), dadd((size_t)K * B), gadd((size_t)K * B);
  for (auto *v : {&packed, &dadd, &gadd})
    for (double &x : *v)
      if (std::scanf("%lf", &x) != 1)
        return 1;
  sage::hold_packed(packed.data(), dadd.data(), gadd.data(), K, nl, links.data(), B, CS, hold.data());
  for (auto *v : {&packed, &dadd, &gadd})
  {
    for (double x : *v)
      std::printf("%.17g ", x);
    std::printf("\n");
  }
  for (int m = 0; m < 8; ++m)
    for (int r = 0; r < B; ++r)
      std::printf("%d ", (int)sage::row_held(m, r, CS));
  std::printf("\n");
  double da, ga;
  sage::SolvePriors pri{1e-3, 1e4, 1e4, 1.5f, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}};
  const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1f, 0, 0}, code[4] = {0.5f, 0.5f, 0.5f, 0.5f};
  for (int m : {0, 7})
    for (int r = 0; r < B; ++r)
    {
      sage::prior_row(pri, 0, r, CS, pose, 2.0f, code, da, ga, m);
      std::printf("%d ", (int)(da != 0.0 || ga != 0.0));
    }
  std::printf("\n");
  return 0;
}
"""


def test_the_held_rule_on_the_host_copy_of_a_system(tmp_path):
    """damped_system.h, compiled on its own with the host compiler: a held row / column keeps no off-diagonal element in its
    diagonal block and its link blocks, a unit diagonal, a zero right-hand side and no prior; the block solve of such a
    system leaves the held entries at exactly zero and gives the free ones the step of the system without them."""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    src, exe = tmp_path / "hold_driver.cpp", tmp_path / "hold_driver"
    src.write_text(HOLD_DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    K, CS = 4, 4
    B, links = 7 + CS, [(0, 1), (1, 2), (0, 2), (2, 3), (0, 1)]     # (a duplicate link: the host path's case)
    hold = [7, 2, 0, 5]
    rng = np.random.default_rng(3)
    n = K * B
    J = rng.normal(size=(3 * n, n))
    H = J.T @ J
    diag = np.stack([H[k * B:(k + 1) * B, k * B:(k + 1) * B] for k in range(K)])
    lnk = np.stack([0.5 * H[a * B:(a + 1) * B, b * B:(b + 1) * B] if (a, b) == (0, 1) else H[a * B:(a + 1) * B, b * B:(b + 1) * B]
                    for a, b in links])
    g = rng.normal(size=n)
    packed = np.concatenate([diag.ravel(), lnk.ravel(), g])
    dadd, gadd = rng.uniform(0.1, 1.0, n), rng.normal(size=n)
    text = " ".join(map(str, [K, len(links), B, CS] + [v for l in links for v in l] + hold)) + " " + \
        " ".join(repr(float(x)) for x in np.concatenate([packed, dadd, gadd]))
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.strip().split("\n")
    pm, dm, gm = (np.array(row.split(), np.float64) for row in rows[:3])
    flags = np.array(rows[3].split(), int).reshape(8, B)
    for m in range(8):
        want = [bool(m & 1)] * 6 + [bool(m & 2)] * CS + [bool(m & 4)]
        assert list(flags[m].astype(bool)) == want, m
    pri = np.array(rows[4].split(), int).reshape(2, B)
    assert pri[0].all() and not pri[1].any()                     # keyframe 0 has a prior on every row; none when held
    held = np.array([k * B + r for k in range(K) for r in range(B) if flags[hold[k]][r]])
    free = np.setdiff1d(np.arange(n), held)
    assert len(held) == 11 + CS + 7 and np.array_equal(pm.shape, packed.shape)
    Hm, gmv, _ = capi.unpack_dense(np.concatenate([pm, np.zeros(4)]), K, links, CS)
    assert np.array_equal(Hm[np.ix_(held, held)], np.eye(len(held)))
    assert not Hm[np.ix_(held, free)].any() and not Hm[np.ix_(free, held)].any() and not gmv[held].any()
    assert not dm[held].any() and not gm[held].any()
    H0, g0, _ = capi.unpack_dense(np.concatenate([packed, np.zeros(4)]), K, links, CS)
    assert np.array_equal(Hm[np.ix_(free, free)], H0[np.ix_(free, free)]) and np.array_equal(gmv[free], g0[free])
    assert np.array_equal(dm[free], dadd[free]) and np.array_equal(gm[free], gadd[free])
    damp = 1e-2
    delta = capi.block_solve(pm, K, links, B, damp, dm, gm)
    A = H0[np.ix_(free, free)] + np.diag(dadd[free])
    ref = np.linalg.solve(A + damp * np.diag(np.diag(A)), (g0 + gadd)[free])
    assert np.all(delta[held] == 0.0)
    assert np.linalg.norm(delta[free] - ref) <= 1e-10 * np.linalg.norm(ref)
