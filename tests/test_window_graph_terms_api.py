"""Pose-graph terms of a window (sage_window_add_graph_term), the parts that need no GPU: header, exports and the ctypes
mirror; argument checks that come before any device call; the numpy restatement (tests/graph_term_ref.py) against central
differences of its own residuals; csrc/graph_terms.h compiled with the host compiler against the restatement.

Measured (fp64 restatement vs central differences, h = 1e-6, unit-scale inputs): <= 3.9e-10 over all 14 columns, both
binary kinds, theta in {0, 1e-4, 1e-2, 1, 2.5}; bar 1e-7 (the rest is h^2 and 1e-16 / h).
graph_terms.h on the host (fp32) against the fp64 restatement over the off-target cases: AtA 7.7e-8, Atb 2.3e-7, error 2.5e-7
rel-L2, where the fp32 restatement itself sits at 6.6e-8 / 1.8e-7 / 8.4e-8 (bars: 2e-6, the floor)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import graph_term_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage_slam_amd", "csrc")
INVALID = -1
NEW = ("sage_window_add_graph_term", "sage_window_num_graph_terms", "sage_window_get_graph_term")


def test_header_declares_and_library_exports_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"SAGE_GRAPH_REL_POSE_SCALE\s*=\s*0\s*,\s*SAGE_GRAPH_REL_POSE\s*=\s*1\s*,\s*SAGE_GRAPH_SCALE_PRIOR\s*=\s*2", hdr)
    assert (capi.SAGE_GRAPH_REL_POSE_SCALE, capi.SAGE_GRAPH_REL_POSE, capi.SAGE_GRAPH_SCALE_PRIOR) == (0, 1, 2)
    assert capi.GRAPH_KINDS == G.KINDS and capi.GRAPH_KIND_ROWS == G.ROWS and capi.GRAPH_TERM_DIM == G.D
    body = re.search(r"typedef struct SageGraphTerm[^{]*\{(.*?)\}\s*SageGraphTerm;", hdr, re.S)
    decl = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*[;,]", decl)
    want = [(n, str(t._length_) if hasattr(t, "_length_") else "") for n, t in capi.SageGraphTerm._fields_]
    assert fields == want                                         # field by field, array lengths included
    for ctype, names in ((r"int32_t", ("kind", "edge", "kf")), (r"float", ("target_pose10", "target_scale0", "weight"))):
        for n in names:
            assert re.search(ctype + r"[^;]*\b" + n + r"\b", decl), n
    assert C.sizeof(capi.SageGraphTerm) == 3 * 4 + 12 * 4 + 5 * 4
    # the header says where the Jacobian leaves the reference's matrix
    assert "kron(pose0^T, I3)" in hdr and "-t10 / s0^2" in hdr


def test_bad_calls_answer_invalid_without_a_device():
    L = capi.lib()
    t = capi.graph_term_struct(dict(kind="rel_pose_scale", edge=0, weight=1.0))
    assert L.sage_window_add_graph_term(None, C.byref(t)) == INVALID
    assert L.sage_window_add_graph_term(None, None) == INVALID
    assert L.sage_window_num_graph_terms(None) == 0
    A = np.zeros((14, 14), np.float32)
    assert L.sage_window_get_graph_term(None, 0, A.ctypes.data_as(C.POINTER(C.c_float)), None, None) == INVALID


def test_struct_from_dict_fills_what_a_kind_leaves_out():
    t = capi.graph_term_struct(dict(kind="scale_prior", kf=3, target_scale0=1.25, weight=100.0))
    assert (t.kind, t.kf, t.target_scale0, t.weight) == (2, 3, 1.25, 100.0)
    assert list(t.target_pose10) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    t = capi.graph_term_struct(dict(kind=capi.SAGE_GRAPH_REL_POSE, edge=5, target_pose10=np.arange(12), weight=2.0, rot_weight=0.5))
    assert (t.kind, t.edge, t.rot_weight) == (1, 5, 0.5) and list(t.target_pose10) == list(range(12))


# ---------------------------------------------------------------------------------------------- restatement vs differences
def unit_cases(rounded):
    """both binary kinds at every theta, targets 0.05 off in translation, rotation and log-scale; one case on target"""
    rng = np.random.default_rng(11)
    cases = [(th, kind, G.binary_case(rng, th, kind, rounded=rounded)) for th in G.THETAS for kind in ("rel_pose_scale", "rel_pose")]
    cases.append((1.0, "rel_pose_scale", G.binary_case(rng, 1.0, "rel_pose_scale", on_target=True, rounded=rounded)))
    return cases


def test_restatement_matches_central_differences_of_its_own_residuals():
    worst = 0.0
    for th, kind, case in unit_cases(rounded=False):
        J, F = G.jacobian(*case), G.fd_jacobian(*case)
        d = float(np.abs(J - F).max())
        print(f"theta {th:g} {kind}: |J - central differences|_max = {d:.2e}")
        worst = max(worst, d)
        assert d <= 1e-7, (th, kind)
        rows = G.ROWS[G.kind_of(case[0])]
        assert not J[rows:].any() and not F[rows:].any()         # REL_POSE: no seventh row, no scale column
        if kind == "rel_pose":
            assert not J[:, 12:].any()
        assert np.abs(J[:, 6:12] + J[:, :6]).max() <= 1e-12       # the pose1 block, derived on its own: minus the pose0 block
    t = dict(kind="scale_prior", kf=0, target_scale0=1.4, weight=100.0)
    J, F = G.jacobian(t, None, None, 1.1, 1.1), G.fd_jacobian(t, np.zeros(12), np.zeros(12), 1.1, 1.1)
    assert np.abs(J - F).max() <= 1e-7 and np.count_nonzero(J) == 1 and J[6, 12] == 1 / 1.1
    lin = G.linearize(t, None, None, 1.1, 1.1)
    assert lin["AtA"][12, 12] == pytest.approx(100.0 / 1.1 ** 2, rel=1e-14) and np.count_nonzero(lin["AtA"]) == 1
    assert lin["Atb"][12] == pytest.approx(100.0 / 1.1 * (np.log(1.4) - np.log(1.1)), rel=1e-14)
    assert lin["error"] == pytest.approx(100.0 * (np.log(1.4) - np.log(1.1)) ** 2, rel=1e-14)
    print(f"worst over the cases: {worst:.2e}")


def test_the_log_is_exact_at_the_identity_and_the_reference_matrix_is_not_the_derivative():
    assert np.array_equal(G.so3_log(np.eye(3)), np.zeros(3)) and np.array_equal(G.so3_log(np.eye(3), np.float32), np.zeros(3))
    # the two places where the reference's matrix leaves the derivative, on one unit-scale case: its pose1 block is not
    # minus the pose0 block (kron without the transpose), and its scale0 column carries the target's translation
    rng = np.random.default_rng(5)
    term, p0, p1, s0, s1 = G.binary_case(rng, 1.0, "rel_pose_scale", rounded=False)
    F = G.fd_jacobian(term, p0, p1, s0, s1)
    assert np.abs(F[:, 6:12] + F[:, :6]).max() <= 1e-7
    as_written_scale0 = -np.asarray(term["target_pose10"], np.float64)[9:] / s0 ** 2
    assert np.abs(F[:3, 12] - as_written_scale0).max() > 1e-2
    assert np.abs(F[:3, 12] + G.relative_pose12(p0, p1)[9:] / s0 ** 2).max() <= 1e-7


# ---------------------------------------------------------------------------------------------- graph_terms.h on the host
DRIVER = r"""
#include "graph_terms.h"
#include <cstdio>
// stdin, per case: kind, pose0 [12], pose1 [12], s0, s1, target [12], ts0, ts1, weight, rot_weight, scale_weight
// stdout, per case: J [7][14], r [7], error, AtA [14][14], Atb [14], the error of the error-only instantiation
int main()
{
  int kind;
  while (std::scanf("%d", &kind) == 1)
  {
    sage::GraphTerm t{};
    t.kind = kind;
    float p0[12], p1[12], s0, s1;
    for (float &v : p0)
      if (std::scanf("%f", &v) != 1)
        return 1;
    for (float &v : p1)
      if (std::scanf("%f", &v) != 1)
        return 1;
    if (std::scanf("%f %f", &s0, &s1) != 2)
      return 1;
    for (float &v : t.target)
      if (std::scanf("%f", &v) != 1)
        return 1;
    if (std::scanf("%f %f %f %f %f", &t.ts0, &t.ts1, &t.weight, &t.rot_weight, &t.scale_weight) != 5)
      return 1;
    float J[sage::kGraphRows][sage::kGraphD], r[sage::kGraphRows], J2[sage::kGraphRows][sage::kGraphD], r2[sage::kGraphRows];
    const float e = sage::graph_term_eval<true>(p0, p1, s0, s1, t, J, r);
    const float e2 = sage::graph_term_eval<false>(p0, p1, s0, s1, t, J2, r2);
    for (auto &row : J)
      for (float v : row)
        std::printf("%.9g ", v);
    for (float v : r)
      std::printf("%.9g ", v);
    std::printf("%.9g ", e);
    float b[sage::kGraphD];
    for (int i = 0; i < sage::kGraphD; ++i)
    {
      float row[sage::kGraphD];
      sage::graph_normal_row(J, r, t.weight, i, row, b[i]);
      for (float v : row)
        std::printf("%.9g ", v);
    }
    for (float v : b)
      std::printf("%.9g ", v);
    std::printf("%.9g\n", e2);
  }
  return 0;
}
"""


def header_cases():
    """the unit-scale cases on fp32 poses, the same with scales 1.3 / 0.8, and scale priors"""
    rng = np.random.default_rng(12)
    cases = [c for _, _, c in unit_cases(rounded=True)]
    cases += [G.binary_case(rng, th, kind, s0=1.3, s1=0.8) for th in G.THETAS for kind in ("rel_pose_scale", "rel_pose")]
    cases.append(G.binary_case(rng, 2.5, "rel_pose", s0=1.3, s1=0.8, on_target=True))
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    for ts, s in ((1.4, 1.1), (0.7, 0.7)):
        cases.append((dict(kind="scale_prior", kf=0, target_pose10=eye, target_scale0=ts, target_scale1=1.0, weight=100.0,
                           rot_weight=1.0, scale_weight=1.0), eye, eye, float(np.float32(s)), float(np.float32(s))))
    return cases


def test_graph_terms_header_on_the_host_matches_the_restatement(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler installed")
    src, exe = tmp_path / "graph_driver.cpp", tmp_path / "graph_driver"
    src.write_text(DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = header_cases()
    lines = []
    for term, p0, p1, s0, s1 in cases:
        nums = [G.kind_of(term)] + list(p0) + list(p1) + [s0, s1] + list(np.asarray(term["target_pose10"], np.float64)) + \
            [term["target_scale0"], term["target_scale1"], term["weight"], term["rot_weight"], term["scale_weight"]]
        lines.append(" ".join(repr(float(v)) if i else str(int(v)) for i, v in enumerate(nums)))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [np.array(l.split(), np.float64) for l in out.stdout.strip().split("\n")]
    assert len(rows) == len(cases) and all(len(v) == 98 + 7 + 1 + 196 + 14 + 1 for v in rows)
    got = [dict(J=v[:98].reshape(7, 14), r=v[98:105], error=v[105], AtA=v[106:302].reshape(14, 14), Atb=v[302:316], error2=v[316])
           for v in rows]
    ref = [G.linearize(*c) for c in cases]
    off = [i for i, c in enumerate(cases) if float(ref[i]["error"]) > 1e-6]
    bars, d32 = G.parity_bars([cases[i] for i in off])
    dist = {k: G.rel_l2(np.concatenate([np.ravel(got[i][k]) for i in off]), np.concatenate([np.ravel(ref[i][k]) for i in off]))
            for k in ("AtA", "Atb", "error")}
    print("graph_terms.h on the host vs fp64 restatement:", {k: f"{v:.2e}" for k, v in dist.items()},
          "fp32 restatement:", {k: f"{v:.2e}" for k, v in d32.items()}, "bars:", {k: f"{v:.2e}" for k, v in bars.items()})
    for k in dist:
        assert dist[k] <= bars[k], (k, dist[k], bars[k])
    for i, (c, g, o) in enumerate(zip(cases, got, ref)):
        assert g["error"] == g["error2"], i                         # the error-only instantiation: the same bits
        assert np.abs(g["J"] - o["J"]).max() <= 2e-6 * max(1.0, np.abs(o["J"]).max()), i
        assert np.array_equal(g["AtA"], g["AtA"].T) or np.abs(g["AtA"] - g["AtA"].T).max() <= 1e-6 * np.abs(g["AtA"]).max()
        rows_ = G.ROWS[G.kind_of(c[0])]
        if G.kind_of(c[0]) == 1:
            assert not g["J"][6].any() and not g["J"][:, 12:].any() and not g["AtA"][12:].any() and not g["Atb"][12:].any()
        if G.kind_of(c[0]) == 2:
            assert np.count_nonzero(g["AtA"]) == 1 and g["AtA"][12, 12] != 0 and np.count_nonzero(g["Atb"]) <= 1
        assert rows_ == 7 or not (g["r"][6:] if rows_ == 6 else g["r"][:6]).any()
        if i not in off:                                            # on target
            assert 0.0 <= g["error"] <= G.on_target_bound(c[0]), (i, g["error"])
    assert len(off) < len(cases)
    # identity relative rotation: the rotation residual of an on-target term at theta = 0 is exactly zero
    rng = np.random.default_rng(2)
    term, p0, p1, s0, s1 = G.binary_case(rng, 0.0, "rel_pose", on_target=True)
    assert np.array_equal(G.residuals(term, p0, p1, s0, s1, np.float32)[3:6], np.zeros(3, np.float32))
