"""One metric for a factor's normal equations: entry by entry, scaled by the reference's own diagonal.

Host only (numpy), no engine import.  The whole-matrix ``rel(AtA, oracle)`` of tests/helpers.py is a Frobenius norm, and
the systems mix units: pose rows of the photometric and reprojection factors are 1e4 .. 1e5, code rows 1e-1, so that norm
is the pose block and little else (the code x code block is 1e-6 .. 8e-6 of it: zeroing it passes 2e-5).  Here every entry
is scaled to a correlation

    dist_A(A, A*)     = max_ij |A_ij - A*_ij| / sqrt(A*_ii A*_jj)
    dist_b(b, A*, b*) = max_i  |b_i - b*_i| / sqrt(A*_ii)   /   max_j |b*_j| / sqrt(A*_jj)

Both are invariant under any rescaling of the variables, and both are bounded by accumulation error without a cancellation
term: a scaled entry of A* is a correlation of two Jacobian columns (|.| <= 1), a scaled entry of b* the projection of the
residual on a unit column.  Where A*_ii = 0 (a column the factor does not have, a factor without inliers) the row, the
column and b_i of the compared system must be EXACTLY zero; such entries then leave the maximum, and a nonzero one makes the
distance infinite.

The functions return a ``Report``: the distance, the worst entry by segment name and index, and per pair of segments the
worst scaled entry; ``str(report)`` prints all of it, and ``check(...)`` is the assertion the tests use -- a failure names
the tile.

Segment tables: the layouts the C ABI hands out (include/sage_ba.h).

Bars.  The constants below are the fp32 oracle's own distance from the fp64 oracle, worst case per factor family over the
case tables of tests/metric_cases.py, times a margin below 2: tests/test_system_metric.py measures them on the CPU and
asserts  measured <= constant <= 2 x measured.  The bar of a kernel against the fp64 oracle is ``BAR_FACTOR`` = 4 times the
constant: the kernels sum fp32 tiles of 64 and 256 samples and then partial records, the oracle in sequence; the fp32-fp64
distance is one draw of that rounding noise, not its bound.
"""
import numpy as np

BAR_FACTOR = 4.0

# fp32 oracle vs fp64 oracle, worst case of the family (tests/test_system_metric.py keeps each within 1x .. 2x of what it
# measures; the measured values are in its output and in DESIGN s4)
FAMILY = {
    # family:                  (dist_A,  dist_b)
    "photometric":            (2.4e-6, 8.5e-6),     # worst: FS = 32, N = 50 (code0 x code0); the FS = 32 window (pose0)
    "geometric":              (8.0e-7, 8.5e-6),
    "merged_pair":            (1.2e-6, 8.5e-6),     # photometric + geometric edge of one directed pair, summed
    "window":                 (9.5e-7, 1.2e-6),     # the K*B system of every edge of a window
    "reprojection":           (2.7e-6, 2.4e-6),     # worst: N = 1
    "tracker_reprojection":   (2.2e-6, 1.05e-5),
    "match_geometry":         (9.8e-7, 3.8e-7),
    "loop_mg":                (2.3e-7, 1.6e-7),
    "tracker_match_geometry": (1.1e-7, 1.3e-7),
    "tracker_photometric":    (9.1e-7, 3.4e-6),
    "window_reprojection":    (1.9e-6, 2.3e-6),     # the window's keypoint terms (tests/test_gpu_window_keypoints.py)
    "window_match_geometry":  (6.5e-7, 1.15e-5),    # dist_b: a CS16 term whose gradient nearly vanishes next to its columns
    "graph_terms":            (5.3e-7, 1.2e-5),     # D = 14 terms: the fp32 restatement of tests/graph_term_ref.py against its fp64
}


def bar_A(family):
    return BAR_FACTOR * FAMILY[family][0]


def bar_b(family):
    return BAR_FACTOR * FAMILY[family][1]


# ---------------------------------------------------------------------------------------------------------------------
# segment tables: [(name, start, stop)]
# ---------------------------------------------------------------------------------------------------------------------
def _table(parts):
    out, at = [], 0
    for name, n in parts:
        out.append((name, at, at + n))
        at += n
    return out


def seg_photo(CS):
    """D = 13+CS [pose0 pose1 code0 scale0]: photometric edge, reprojection term"""
    return _table([("pose0", 6), ("pose1", 6), ("code0", CS), ("scale0", 1)])


def seg_geo(CS):
    """D = 14+2CS [pose0 pose1 code0 code1 scale0 scale1]: geometric edge, match-geometry term"""
    return _table([("pose0", 6), ("pose1", 6), ("code0", CS), ("code1", CS), ("scale0", 1), ("scale1", 1)])


def seg_loop():
    """D = 14 [pose0 pose1 scale0 scale1]: loop match geometry, graph terms"""
    return _table([("pose0", 6), ("pose1", 6), ("scale0", 1), ("scale1", 1)])


def seg_tracker(dof):
    """D = 6 [pose] / D = 7 [pose scale]: the tracker"""
    assert dof in (6, 7)
    return _table([("pose", 6)] + ([("scale", 1)] if dof == 7 else []))


def seg_window(K, CS):
    """the window's K*B system, B = 7+CS: [pose(6) code(CS) scale] per keyframe"""
    return _table([(f"{n}[{k}]", m) for k in range(K) for n, m in (("pose", 6), ("code", CS), ("scale", 1))])


def segments_for(D):
    """the per-edge layout of a D x D system with CS in (16, 32) (the sizes are distinct)"""
    for CS in (16, 32):
        if D == 13 + CS:
            return seg_photo(CS)
        if D == 14 + 2 * CS:
            return seg_geo(CS)
    if D == 14:
        return seg_loop()
    if D in (6, 7):
        return seg_tracker(D)
    raise ValueError(f"no per-edge layout has D = {D}")


def segment(segs, name):
    for n, a, b in segs:
        if n == name:
            return np.arange(a, b)
    raise KeyError(name)


def _locate(segs, i):
    for n, a, b in segs:
        if a <= i < b:
            return n, int(i - a)
    raise IndexError(i)


# ---------------------------------------------------------------------------------------------------------------------
class Report:
    """dist: the distance (inf where an entry that must be exactly zero is not).  worst: (row name, row index in its segment,
    column name, column index, scaled difference) -- for dist_b (name, index, scaled difference).  blocks: {(row segment,
    column segment): worst scaled difference} (dist_b: {segment: ...}).  nonzero: entries that had to be exactly zero."""

    def __init__(self, what, dist, worst, blocks, nonzero, unit=1.0):
        self.what, self.dist, self.worst, self.blocks, self.nonzero, self.unit = what, float(dist), worst, blocks, nonzero, unit

    def __float__(self):
        return self.dist

    def worst_name(self):
        return "x".join(str(v) for v in self.worst[:-1:2]) if self.worst else ""

    def __str__(self):
        lines = [f"{self.what} = {self.dist:.3e}"]
        if self.worst:
            if len(self.worst) == 5:
                lines.append(f"  worst entry: {self.worst[0]}[{self.worst[1]}] x {self.worst[2]}[{self.worst[3]}]  "
                             f"scaled difference {self.worst[4]:.3e}")
            else:
                lines.append(f"  worst entry: {self.worst[0]}[{self.worst[1]}]  scaled difference {self.worst[2]:.3e}")
        for e in self.nonzero[:8]:
            lines.append(f"  must be exactly zero (zero reference diagonal) but is {e[-1]:.3e}: {e[:-1]}")
        lines.append("  worst scaled entry per block:")
        for key, v in sorted(self.blocks.items(), key=lambda kv: -kv[1]):
            name = " x ".join(key) if isinstance(key, tuple) else key
            lines.append(f"    {name:28s} {v:.3e}")
        return "\n".join(lines)


def _as64(x):
    return np.asarray(x, np.float64)


def dist_A(A, A_ref, segs=None):
    A, R = _as64(A), _as64(A_ref)
    assert A.shape == R.shape and A.ndim == 2 and A.shape[0] == A.shape[1], (A.shape, R.shape)
    D = A.shape[0]
    segs = segments_for(D) if segs is None else segs
    assert segs[-1][2] == D
    d = np.diag(R)
    assert (d >= 0).all(), "the reference's diagonal is negative"
    live = d > 0
    s = np.sqrt(np.where(live, d, 1.0))
    both = np.outer(live, live)
    scaled = np.where(both, np.abs(A - R) / np.outer(s, s), 0.0)
    nonzero = [(*_locate(segs, i), *_locate(segs, j), float(A[i, j])) for i, j in zip(*np.nonzero((A != 0) & ~both))]
    blocks = {}
    for n1, a1, b1 in segs:
        for n2, a2, b2 in segs:
            if a2 < a1:
                continue
            blk = scaled[a1:b1, a2:b2]
            v = float(max(blk.max(), scaled[a2:b2, a1:b1].max())) if blk.size else 0.0
            blocks[(n1, n2)] = v
    i, j = np.unravel_index(int(np.argmax(scaled)), scaled.shape)
    worst = (*_locate(segs, i), *_locate(segs, j), float(scaled[i, j]))
    dist = np.inf if nonzero or not np.isfinite(A).all() else float(scaled.max())
    return Report("dist_A", dist, worst, blocks, nonzero)


def dist_b(b, A_ref, b_ref, segs=None):
    b, R, r = _as64(b), _as64(A_ref), _as64(b_ref)
    assert b.shape == r.shape and b.ndim == 1 and R.shape == (b.size, b.size), (b.shape, r.shape, R.shape)
    D = b.size
    segs = segments_for(D) if segs is None else segs
    assert segs[-1][2] == D
    d = np.diag(R)
    live = d > 0
    s = np.sqrt(np.where(live, d, 1.0))
    unit = float(np.max(np.where(live, np.abs(r) / s, 0.0)))
    diff = np.where(live, np.abs(b - r) / s, 0.0)
    nonzero = [(*_locate(segs, i), float(b[i])) for i in np.nonzero((b != 0) & ~live)[0]]
    if unit > 0:
        scaled = diff / unit
    else:                                            # a zero reference gradient: only an exact zero is at distance 0
        scaled = np.where(diff > 0, np.inf, 0.0)
    blocks = {n: float(scaled[a:c].max()) for n, a, c in segs if c > a}
    i = int(np.argmax(scaled))
    worst = (*_locate(segs, i), float(scaled[i]))
    dist = np.inf if nonzero or not np.isfinite(b).all() else float(scaled.max())
    return Report("dist_b", dist, worst, blocks, nonzero, unit)


WORST = {}      # family -> [worst dist_A, its label and entry, worst dist_b, its label and entry, systems checked]


def check(h, o64, family, label="", segs=None, against="the fp64 oracle"):
    """the GPU tests' assertion: AtA / Atb of ``h`` against the fp64 oracle's ``o64`` under the family's bars; a failure
    prints the reports.  The worst distances per family are kept for ``summary_lines``; ``against`` names another reference
    (two engine paths against each other) and keeps those apart.  -> (dist_A report, dist_b report)"""
    ra = dist_A(_host(h["AtA"]), o64["AtA"], segs)
    rb = dist_b(_host(h["Atb"]), o64["AtA"], o64["Atb"], segs)
    w = WORST.setdefault((family, against), [0.0, "", 0.0, "", 0])
    if ra.dist >= w[0]:
        w[0], w[1] = ra.dist, f"{label} {ra.worst_name()}"
    if rb.dist >= w[2]:
        w[2], w[3] = rb.dist, f"{label} {rb.worst_name()}"
    w[4] += 1
    assert ra.dist < bar_A(family), f"{family} {label}: dist_A over its bar {bar_A(family):.2e}\n{ra}"
    assert rb.dist < bar_b(family), f"{family} {label}: dist_b over its bar {bar_b(family):.2e}\n{rb}"
    return ra, rb


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def summary_lines(where):
    """one line per family checked since the last call: the kernels' worst distances from the fp64 oracle next to the bars"""
    out = []
    for (family, against), (a, la, b, lb, n) in sorted(WORST.items()):
        out.append(f"[system metric, {where}] {family}: {n} systems vs {against}, worst dist_A {a:.2e} = {a / bar_A(family):.2f} bar "
                   f"({la.strip()}), dist_b {b:.2e} = {b / bar_b(family):.2f} bar ({lb.strip()}); bars {bar_A(family):.1e} / {bar_b(family):.1e}")
    WORST.clear()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the mutants of tests/test_system_metric.py: each returns a changed copy
# ---------------------------------------------------------------------------------------------------------------------
def code_segments(segs):
    return [(n, a, b) for n, a, b in segs if n.startswith("code")]


def mutant_code_code_zeroed(A, segs):
    """(a) every code x code block zeroed"""
    A = np.array(A, np.float64)
    cs = code_segments(segs)
    for _, a1, b1 in cs:
        for _, a2, b2 in cs:
            A[a1:b1, a2:b2] = 0
    return A


def mutant_code_tile(A, seg, f=1.001):
    """(b) one 16 x 16 code tile x f: the high x high tile of a CS = 32 segment, the only one of CS = 16"""
    A = np.array(A, np.float64)
    _, a, b = seg
    A[b - 16:b, b - 16:b] *= f
    return A


def mutant_pose_code_high(A, seg, f=1.001):
    """(c) pose x code-high (the last 16 code columns) x f, mirrored"""
    A = np.array(A, np.float64)
    _, a, b = seg
    pose = _pose_rows_of(seg)
    A[np.ix_(pose, np.arange(b - 16, b))] *= f
    A[np.ix_(np.arange(b - 16, b), pose)] *= f
    return A


def _pose_rows_of(seg):
    """pose rows a code segment goes with: per-edge layouts [0, 12), the window's keyframe: the 6 before its code"""
    n, a, b = seg
    return np.arange(a - 6, a) if n.startswith("code[") else np.arange(12)


def mutant_last_code(A, seg, f=1.001):
    """(d) the last code row and column x f (the diagonal entry once)"""
    A = np.array(A, np.float64)
    i = seg[2] - 1
    d = A[i, i]
    A[i, :] *= f
    A[:, i] *= f
    A[i, i] = d * f
    return A


def mutant_code_scale(A, seg, scale_idx, f=1.001):
    """(e) code x scale x f, mirrored"""
    A = np.array(A, np.float64)
    _, a, b = seg
    A[np.ix_(np.arange(a, b), scale_idx)] *= f
    A[np.ix_(scale_idx, np.arange(a, b))] *= f
    return A


def mutant_b_code(b, seg, f=1.01):
    """(f) the Atb code segment x f"""
    b = np.array(b, np.float64)
    b[seg[1]:seg[2]] *= f
    return b


def scale_indices(segs, seg):
    """the scale columns a code segment's factor has: all of a per-edge layout, the keyframe's own in the window"""
    n = seg[0]
    if n.startswith("code["):
        return segment(segs, "scale" + n[4:])
    return np.concatenate([np.arange(a, b) for m, a, b in segs if m.startswith("scale")])
