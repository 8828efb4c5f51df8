"""The entry-by-entry system metric (tests/system_metric.py) on the CPU, with the oracle alone: nothing here knows a kernel.

1. The families' constants.  For every system of every case table (tests/metric_cases.py) dist_A and dist_b of the fp32
   oracle against the fp64 oracle -- the reference's own arithmetic against the exact value.  The worst per family is what
   the committed constant stands for:  measured <= constant <= 2 x measured, so a constant neither goes stale nor loose.
   Measured here (dist_A / dist_b, the case that sets it):
     photometric             1.87e-6 (32x40 FS32 CS32 N50 0->1, code0 x code0) / 6.69e-6 (FS = 32 window, CS32, 0->1, pose0)
     geometric               6.13e-7 (border 64x80 window 3->1)                / 6.58e-6 (K = 5 window CS16, 2->3)
     merged_pair             9.03e-7 (FS = 32 window CS16, 2->1, code0 x code0) / 6.69e-6 (FS = 32 window CS32, 0->1)
     window                  7.35e-7 (K = 5, CS32) / 9.49e-7 (FS = 32 window, CS32)
     reprojection            2.07e-6 (CS32 N = 1)  / 1.86e-6 (CS16 N = 1000)
     tracker_reprojection    1.67e-6 (N = 1)       / 8.23e-6 (N = 1000)
     match_geometry          7.51e-7 (CS16 N40, huber with a zero difference) / 2.90e-7
     loop_mg                 1.77e-7 / 1.24e-7
     tracker_match_geometry  8.43e-8 / 1.00e-7
     tracker_photometric     7.02e-7 (32x40 FS32 N63 dof 7) / 2.61e-6 (64x80 FS32 N700 dof 6)
     window_reprojection     1.49e-6 (CS16, edge 22) / 1.78e-6 (CS32, edge 4)
     window_match_geometry   5.00e-7 (N = 1 term)    / 9.00e-6 (CS16 fair, edge 8)
     graph_terms             4.11e-7 / 9.35e-6 (the fp32 restatement of tests/graph_term_ref.py against its fp64 one)

2. The metric sees what the whole-matrix norm misses.  On the fp64 oracle's output of every system that has a code segment,
   the mutants (a) code x code zeroed, (b) one 16 x 16 code tile x 1.001, (c) pose x code-high x 1.001 (mirrored), (d) the last
   code row and column x 1.001, (e) code x scale x 1.001, (f) the Atb code segment x 1.01 -- per code segment of the layout
   (the geometric layouts have two, the window one per keyframe).  Every mutant must be at least 10 bars away (bar = 4 x the
   family's constant).  The old whole-matrix rel-L2 of the same mutant is collected and printed.  Measured here, least
   distance in bars over the family's systems | the old rel-L2 of the mutant, min .. max (the old bar is 2e-5):
                       photometric (101 systems)      reprojection (7)            window K*B (7)
     (a)            1.0e5 | 6.2e-7 .. 9.4e-5      9.3e4 | 6.0e-6 .. 7.9e-5     2.6e5 | 3.6e-6 .. 3.5e-5
     (b)              104 | 6.2e-10 .. 5.4e-8        93 | 5.9e-9 .. 4.2e-8       263 | 8.8e-10 .. 1.6e-8
     (c)               40 | 4.1e-7 .. 4.4e-6         11 | 3.3e-7 .. 7.9e-6        14 | 1.5e-8 .. 1.1e-6
     (d)              104 | 1.3e-8 .. 1.5e-6         93 | 3.3e-8 .. 1.3e-6       263 | 7.3e-9 .. 3.4e-7
     (e)               50 | 3.1e-9 .. 3.9e-7         14 | 1.0e-8 .. 3.2e-7       127 | 5.3e-9 .. 1.2e-7
     (f)               28 | 1.3e-6 .. 2.5e-4        634 | 2.6e-5 .. 2.2e-4        74 | 4.4e-7 .. 1.8e-5
   so on the photometric, reprojection and window systems mutants (b) .. (e) changed no old assertion on any case, and (a) only
   on a few.  The geometric and match-geometry layouts have their code rows in the units of the pose rows: there the old norm
   saw (a) (6e-3 .. 2e-2) and sometimes (c) .. (e) (2e-6 .. 9e-5), never (b) (<= 6.4e-6); the new distance is 20 .. 385 bars.
   Left out: no case for (a) .. (e); nothing was skipped by the rule of (f) (a code segment whose components of
   b* / sqrt(diag A*) are all below 1e-2 of the largest).  Another seed: the reprojection scene (CS 32, N 300), see
   tests/metric_cases.REPROJ_SEEDS.  The summed pair is mutated on code0 only: NOT_MUTATED below.
"""
import numpy as np
import pytest

from tests import metric_cases as mc
from tests import system_metric as sm
from tests.helpers import rel

OLD_BAR = 2e-5


@pytest.fixture(scope="module")
def systems(orc):
    """{family: [(label, segments, fp32 oracle, fp64 oracle)]}, computed once and left unchanged"""
    return {f: list(mc.family_cases(orc, f)) for f in mc.FAMILIES}


# ------------------------------------------------------------------------------------------------------ the metric itself
def _random_system(rng, D, n=200):
    J = rng.standard_normal((n, D)) * np.logspace(-3, 3, D)
    r = rng.standard_normal(n)
    return J.T @ J, J.T @ r


def test_invariant_under_rescaling_of_the_variables():
    rng = np.random.default_rng(0)
    A, b = _random_system(rng, 45)
    A2 = A * (1 + 1e-5 * rng.standard_normal(A.shape)); A2 = 0.5 * (A2 + A2.T)
    b2 = b * (1 + 1e-5 * rng.standard_normal(b.shape))
    s = np.logspace(-4, 5, 45)[rng.permutation(45)]
    S = np.outer(s, s)
    assert float(sm.dist_A(A2 * S, A * S)) == pytest.approx(float(sm.dist_A(A2, A)), rel=1e-9)
    assert float(sm.dist_b(b2 * s, A * S, b * s)) == pytest.approx(float(sm.dist_b(b2, A, b)), rel=1e-9)
    assert float(sm.dist_A(A, A)) == 0.0 and float(sm.dist_b(b, A, b)) == 0.0


def test_zero_diagonal_demands_exact_zeros():
    rng = np.random.default_rng(1)
    A, b = _random_system(rng, 14)
    A[12:] = 0; A[:, 12:] = 0; b[12:] = 0            # a factor without scale columns
    assert float(sm.dist_A(A, A)) == 0.0 and float(sm.dist_b(b, A, b)) == 0.0
    A2 = A.copy(); A2[3, 13] = 1e-30
    ra = sm.dist_A(A2, A)
    assert ra.dist == np.inf and ra.nonzero == [("pose0", 3, "scale1", 0, 1e-30)] and "must be exactly zero" in str(ra)
    b2 = b.copy(); b2[12] = -1e-30
    rb = sm.dist_b(b2, A, b)
    assert rb.dist == np.inf and rb.nonzero == [("scale0", 0, -1e-30)]
    # the dead entries leave the maximum: a live difference is still what is reported
    A3 = A.copy(); A3[2, 7] *= 1.01; A3[7, 2] *= 1.01
    assert sm.dist_A(A3, A).worst[:4] in (("pose0", 2, "pose1", 1), ("pose1", 1, "pose0", 2))
    # NaN is no distance
    A4 = A.copy(); A4[0, 0] = np.nan
    assert sm.dist_A(A4, A).dist == np.inf
    # an all-zero reference gradient: only an exact zero is at distance 0
    z = np.zeros_like(b)
    assert float(sm.dist_b(z, A, z)) == 0.0 and sm.dist_b(b * 1e-20, A, z).dist == np.inf


def test_report_names_the_tile():
    rng = np.random.default_rng(2)
    A, b = _random_system(rng, 45)
    segs = sm.seg_photo(32)
    m = sm.mutant_code_tile(A, segs[2])
    r = sm.dist_A(m, A)
    assert r.worst[0] == "code0" and r.worst[2] == "code0" and r.worst[1] >= 16 and r.worst[3] >= 16
    assert r.worst_name() == "code0xcode0"
    assert max(r.blocks, key=r.blocks.get) == ("code0", "code0") and r.blocks[("pose0", "pose0")] == 0.0
    text = str(r)
    assert "worst entry: code0[" in text and "code0 x code0" in text and "pose0 x scale0" in text
    rb = sm.dist_b(sm.mutant_b_code(b, segs[2]), A, b)
    assert rb.worst[0] == "code0" and set(rb.blocks) == {"pose0", "pose1", "code0", "scale0"}


def test_segment_tables_cover_every_layout():
    for D, names in ((45, "pose0 pose1 code0 scale0"), (29, "pose0 pose1 code0 scale0"),
                     (78, "pose0 pose1 code0 code1 scale0 scale1"), (46, "pose0 pose1 code0 code1 scale0 scale1"),
                     (14, "pose0 pose1 scale0 scale1"), (6, "pose"), (7, "pose scale")):
        segs = sm.segments_for(D)
        assert [n for n, _, _ in segs] == names.split() and segs[0][1] == 0 and segs[-1][2] == D
        assert all(a[2] == b[1] for a, b in zip(segs, segs[1:]))
    w = sm.seg_window(3, 16)
    assert w[-1] == ("scale[2]", 68, 69) and w[4] == ("code[1]", 29, 45) and len(w) == 9
    with pytest.raises(ValueError):
        sm.segments_for(13)


# ------------------------------------------------------------------------------------------------------ 1. the constants
def test_every_family_has_cases_and_a_constant(systems):
    assert set(systems) == set(sm.FAMILY) and all(len(v) > 0 for v in systems.values())


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_constant_is_within_1x_and_2x_of_the_measured_distance(systems, family):
    worst = dict(A=(0.0, ""), b=(0.0, ""))
    for label, segs, o32, o64 in systems[family]:
        assert np.diag(o64["AtA"]).max() > 0, label                  # (a case without inliers measures nothing)
        ra = sm.dist_A(o32["AtA"], o64["AtA"], segs)
        rb = sm.dist_b(o32["Atb"], o64["AtA"], o64["Atb"], segs)
        assert np.isfinite(ra.dist) and np.isfinite(rb.dist), f"{label}\n{ra}\n{rb}"
        worst["A"] = max(worst["A"], (ra.dist, f"{label}: {ra.worst_name()}"))
        worst["b"] = max(worst["b"], (rb.dist, f"{label}: {rb.worst_name()}"))
    cA, cb = sm.FAMILY[family]
    print(f"{family}: fp32 oracle vs fp64 oracle over {len(systems[family])} systems: dist_A {worst['A'][0]:.3e} ({worst['A'][1]}), "
          f"constant {cA:.2e};  dist_b {worst['b'][0]:.3e} ({worst['b'][1]}), constant {cb:.2e}")
    assert worst["A"][0] <= cA <= 2 * worst["A"][0], (family, worst["A"], cA)
    assert worst["b"][0] <= cb <= 2 * worst["b"][0], (family, worst["b"], cb)


# ------------------------------------------------------------------------------------------------------ 2. the mutants
MUTANT_FAMILIES = ["photometric", "geometric", "merged_pair", "window", "reprojection", "match_geometry", "window_reprojection",
                   "window_match_geometry"]
F_SKIP_SHARE = 1e-2      # (f) may skip a code segment whose components of b* / sqrt(diag A*) are all below this share

# The merged pair is the photometric and the geometric edge of one directed pair summed: its code1 blocks are the geometric
# edge's alone, mutated at full sensitivity in the "geometric" family.  In the sum the pose columns are the photometric
# edge's (1e4 times larger, no code1 part), so the pose x code1 correlations shrink to 0.024 and a 0.1 % error of that tile
# is 9 of the pair's bars, not 10.  Mutants (b) .. (f) of the pair are those of code0, the segment the merge is about.
NOT_MUTATED = {("merged_pair", "code1")}


def _mutants_of(A, segs, seg):
    yield "b", sm.mutant_code_tile(A, seg)
    yield "c", sm.mutant_pose_code_high(A, seg)
    yield "d", sm.mutant_last_code(A, seg)
    yield "e", sm.mutant_code_scale(A, seg, sm.scale_indices(segs, seg))


@pytest.mark.parametrize("family", MUTANT_FAMILIES)
def test_mutants_are_ten_bars_away(systems, family):
    barA, barb = sm.bar_A(family), sm.bar_b(family)
    old = {k: [np.inf, 0.0] for k in "abcdef"}          # the old whole-matrix rel-L2 of each mutant: [min, max]
    new = {k: np.inf for k in "abcdef"}                 # the new distance in bars: min
    skipped, failures = [], []

    def note(kind, d_new, bars, d_old, where):
        old[kind] = [min(old[kind][0], d_old), max(old[kind][1], d_old)]
        new[kind] = min(new[kind], d_new / bars)
        if not d_new >= 10 * bars:
            failures.append(f"({kind}) {where}: {d_new:.3e} is under 10 bars = {10 * bars:.3e}")

    for label, segs, _, o64 in systems[family]:
        A, b = np.asarray(o64["AtA"], np.float64), np.asarray(o64["Atb"], np.float64)
        codes = sm.code_segments(segs)
        assert codes, label
        m = sm.mutant_code_code_zeroed(A, segs)
        note("a", sm.dist_A(m, A, segs).dist, barA, rel(m, A), label)
        s = np.sqrt(np.diag(A))
        unit = np.max(np.abs(b) / np.where(s > 0, s, np.inf))
        for seg in codes:
            if (family, seg[0]) in NOT_MUTATED:
                continue
            live = s[seg[1]:seg[2]] > 0
            if not live.any():
                continue                                 # (a code segment the factor does not have reads zero: nothing to mutate)
            for kind, m in _mutants_of(A, segs, seg):
                r = sm.dist_A(m, A, segs)
                assert kind == "e" or r.worst[0] == seg[0] or r.worst[2] == seg[0], (label, kind, str(r))
                note(kind, r.dist, barA, rel(m, A), f"{label} {seg[0]}")
            share = np.max(np.abs(b[seg[1]:seg[2]][live]) / s[seg[1]:seg[2]][live]) / unit
            if share < F_SKIP_SHARE:
                skipped.append(f"{label} {seg[0]} (share {share:.1e})")
                continue
            mb = sm.mutant_b_code(b, seg)
            rb = sm.dist_b(mb, A, b, segs)
            assert rb.worst[0] == seg[0]
            note("f", rb.dist, barb, rel(mb, b), f"{label} {seg[0]}")
    print(f"{family}: {len(systems[family])} systems; per mutant: least distance in bars | old whole-matrix rel-L2 min .. max")
    for k in "abcdef":
        print(f"  ({k}) {new[k]:9.1f} bars | {old[k][0]:.2e} .. {old[k][1]:.2e}   (old bar {OLD_BAR:.0e})")
    print(f"  (f) skipped by its rule: {skipped if skipped else 'none'}")
    assert not failures, "\n".join(failures)
