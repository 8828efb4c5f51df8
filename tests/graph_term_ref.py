"""numpy restatement of the window's pose-graph terms (sage_window_add_graph_term): the yardstick of
tests/test_window_graph_terms_api.py (against central differences and against csrc/graph_terms.h compiled on the host) and
of tests/test_gpu_window_graph_terms.py (against the engine).

Every function takes a ``dtype``: np.float64 is the yardstick, np.float32 rounds every intermediate to fp32 -- its distance
from the fp64 result is what fp32 arithmetic costs on the same terms, whatever the order of the operations.

The residuals r = target - current are the reference's as written (rel_pose_scale_factor.cpp:207-227, rel_pose_factor.cpp:
150-170, scale_factor.cpp:102-129); J = d current / d [delta0 delta1 s0 s1] under the left retraction T <- exp(delta) T,
tangent [translation, rotation], is their derivative, written here from the RIGHT Jacobian of SO(3) (the engine uses the left
one) and with the pose1 columns derived on their own (the engine negates the pose0 block).  D = 14 layout for every kind."""
import numpy as np

KINDS = {"rel_pose_scale": 0, "rel_pose": 1, "scale_prior": 2}
ROWS = {0: 7, 1: 6, 2: 1}
D = 14


def kind_of(term):
    return KINDS.get(term["kind"], term["kind"])


def hat(v, dtype=np.float64):
    z = dtype(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype)


def so3_log(R, dtype=np.float64):
    """log of a rotation matrix -> phi [3]; atan2(|sin part|, cos), the series of asin(s) / s next to the identity"""
    R = np.asarray(R, dtype).reshape(3, 3)
    a = dtype(0.5) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype)
    s2 = dtype(a @ a)
    c = dtype(0.5) * (R[0, 0] + R[1, 1] + R[2, 2] - dtype(1))
    if c > 0 and s2 < dtype(1e-4):
        k = dtype(1) + s2 * (dtype(1) / dtype(6) + s2 * (dtype(3) / dtype(40) + s2 * (dtype(5) / dtype(112))))
    else:
        s = np.sqrt(s2)
        k = np.arctan2(s, c) / s
    return (k * a).astype(dtype)


def so3_right_jacobian_inverse(phi, dtype=np.float64):
    """log(R exp(e)) = phi + Jr^-1(phi) e:  Jr^-1 = I + [phi]x / 2 + (1 / th^2 - (1 + cos th) / (2 th sin th)) [phi]x^2"""
    phi = np.asarray(phi, dtype)
    th2 = dtype(phi @ phi)
    if th2 < dtype(1e-4):
        c = dtype(1) / dtype(12) + th2 * (dtype(1) / dtype(720) + th2 * (dtype(1) / dtype(30240)))
    else:
        th = np.sqrt(th2)
        c = dtype(1) / th2 - (dtype(1) + np.cos(th)) / (dtype(2) * th * np.sin(th))
    K = hat(phi, dtype)
    return (np.eye(3, dtype=dtype) + dtype(0.5) * K + c * (K @ K).astype(dtype)).astype(dtype)


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-9:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def retract(pose12, delta6):
    """exp([v, w]) * pose in fp64 (the window's left retraction; the exact SE(3) exponential)"""
    pose12 = np.asarray(pose12, np.float64)
    v, w = np.asarray(delta6[:3], np.float64), np.asarray(delta6[3:], np.float64)
    th = np.linalg.norm(w)
    K = hat(w)
    V = np.eye(3) + 0.5 * K + K @ K / 6.0 if th < 1e-9 else \
        np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
    dR = so3_exp(w)
    R, t = pose12[:9].reshape(3, 3), pose12[9:]
    return np.concatenate([(dR @ R).ravel(), dR @ t + V @ v])


def inverse_target(target12):
    """the target of the opposite direction: (R^T, -R^T t)"""
    R, t = np.asarray(target12[:9], np.float64).reshape(3, 3), np.asarray(target12[9:], np.float64)
    return np.concatenate([R.T.ravel(), -R.T @ t])


def relative_pose12(pose0, pose1):
    """pose1^-1 * pose0 as 12 numbers, fp64"""
    p0, p1 = np.asarray(pose0, np.float64), np.asarray(pose1, np.float64)
    R0, R1 = p0[:9].reshape(3, 3), p1[:9].reshape(3, 3)
    return np.concatenate([(R1.T @ R0).ravel(), R1.T @ (p0[9:] - p1[9:])])


def residuals(term, pose0, pose1, s0, s1, dtype=np.float64):
    """r [7] = target - current (rows a kind does not have: zero)"""
    kind = kind_of(term)
    one = dtype(1)
    r = np.zeros(7, dtype)
    if kind == 2:
        r[6] = np.log(dtype(term["target_scale0"])) - np.log(dtype(s0))
        return r
    p0, p1 = np.asarray(pose0, dtype), np.asarray(pose1, dtype)
    R0, t0, R1, t1 = p0[:9].reshape(3, 3), p0[9:], p1[:9].reshape(3, 3), p1[9:]
    tgt = np.asarray(term["target_pose10"], dtype)
    R10 = (R1.T @ R0).astype(dtype)
    t10 = (R1.T @ (t0 - t1)).astype(dtype)
    s0, s1 = dtype(s0), dtype(s1)
    ts0, ts1 = (dtype(term["target_scale0"]), dtype(term["target_scale1"])) if kind == 0 else (one, one)
    sr = np.sqrt(dtype(term["rot_weight"]))
    if kind == 0:
        r[:3] = tgt[9:] / ts0 - t10 / s0
        r[6] = np.sqrt(dtype(term["scale_weight"])) * (np.log(ts1 / ts0) - np.log(s1 / s0))
    else:
        r[:3] = tgt[9:] - t10
    r[3:6] = sr * (so3_log(tgt[:9], dtype) - so3_log(R10, dtype))
    return r.astype(dtype)


def jacobian(term, pose0, pose1, s0, s1, dtype=np.float64):
    """J [7, 14] = d current / d [delta0 delta1 s0 s1]"""
    kind = kind_of(term)
    J = np.zeros((7, D), dtype)
    if kind == 2:
        J[6, 12] = dtype(1) / dtype(s0)
        return J
    p0, p1 = np.asarray(pose0, dtype), np.asarray(pose1, dtype)
    R0, t0, R1, t1 = p0[:9].reshape(3, 3), p0[9:], p1[:9].reshape(3, 3), p1[9:]
    s0, s1 = dtype(s0), dtype(s1)
    inv = dtype(1) / s0 if kind == 0 else dtype(1)
    sr = np.sqrt(dtype(term["rot_weight"]))
    R10 = (R1.T @ R0).astype(dtype)
    t10 = (R1.T @ (t0 - t1)).astype(dtype)
    Jri = so3_right_jacobian_inverse(so3_log(R10, dtype), dtype)
    # pose0: R10 -> R10 exp(R0^T w0), t10 -> t10 + R1^T (v0 + w0 x t0)
    J[:3, 0:3] = R1.T * inv
    J[:3, 3:6] = -(R1.T @ hat(t0, dtype)) * inv
    J[3:6, 3:6] = sr * (Jri @ R0.T)
    # pose1: R10 -> R10 exp(-R0^T w1), t10 -> t10 - R1^T v1 + R1^T ([t0 - t1]x + [t1]x) w1
    J[:3, 6:9] = -R1.T * inv
    J[:3, 9:12] = (R1.T @ (hat(t0 - t1, dtype) + hat(t1, dtype))) * inv
    J[3:6, 9:12] = -sr * (Jri @ R0.T)
    if kind == 0:
        ss = np.sqrt(dtype(term["scale_weight"]))
        J[:3, 12] = -t10 / (s0 * s0)
        J[6, 12] = -ss / s0
        J[6, 13] = ss / s1
    return J.astype(dtype)


def linearize(term, pose0, pose1, s0, s1, dtype=np.float64):
    """-> dict(AtA [14,14], Atb [14], error, J, r), everything in ``dtype``"""
    r = residuals(term, pose0, pose1, s0, s1, dtype)
    J = jacobian(term, pose0, pose1, s0, s1, dtype)
    w = dtype(term["weight"])
    return dict(AtA=(w * (J.T @ J).astype(dtype)).astype(dtype), Atb=(w * (J.T @ r).astype(dtype)).astype(dtype),
                error=dtype(w * dtype(r @ r)), J=J, r=r)


def error(term, pose0, pose1, s0, s1, dtype=np.float64):
    r = residuals(term, pose0, pose1, s0, s1, dtype)
    return dtype(dtype(term["weight"]) * dtype(r @ r))


def fd_jacobian(term, pose0, pose1, s0, s1, h=1e-6):
    """central differences of -residuals (= the current values, up to the constant target) over the 14 columns, fp64"""
    J = np.zeros((7, D))
    for j in range(D):
        out = []
        for sgn in (1.0, -1.0):
            q0, q1, a0, a1 = np.asarray(pose0, np.float64), np.asarray(pose1, np.float64), float(s0), float(s1)
            d = np.zeros(6)
            if j < 6:
                d[j] = sgn * h
                q0 = retract(q0, d)
            elif j < 12:
                d[j - 6] = sgn * h
                q1 = retract(q1, d)
            elif j == 12:
                a0 += sgn * h
            else:
                a1 += sgn * h
            if kind_of(term) == 2:
                q1, a1 = q0, a0
            out.append(-residuals(term, q0, q1, a0, a1, np.float64))
        J[:, j] = (out[0] - out[1]) / (2 * h)
    return J


def term_keyframes(term, links):
    """(k0, k1) of a term on a window with these links; a scale prior: (kf, kf)"""
    if kind_of(term) == 2:
        return term["kf"], term["kf"]
    a, b = links[term["edge"] // 2]
    return (a, b) if term["edge"] % 2 == 0 else (b, a)


def linearize_on(term, links, poses, scales, dtype=np.float64):
    """a term of a window at variables poses [K][12], scales [K]"""
    k0, k1 = term_keyframes(term, links)
    return linearize(term, poses[k0], poses[k1], scales[k0], scales[k1], dtype)


def place(packed_parts, K, links, CS, term, res):
    """add one term's result (dict AtA, Atb, error) into (diag [K,B,B], lnk [nl,B,B], g [K,B], tail [4]) by hand: pose rows
    0..5 and the scale row 6 + CS of the term's keyframes, nothing else"""
    diag, lnk, g, tail = packed_parts
    A, b = np.asarray(res["AtA"], np.float64), np.asarray(res["Atb"], np.float64)
    rows = list(range(6)) + [6 + CS]
    cols = {0: list(range(6)) + [12], 1: list(range(6, 12)) + [13]}
    k0, k1 = term_keyframes(term, links)
    tail[1] += float(res["error"])
    if kind_of(term) == 2:
        diag[k0][np.ix_(rows, rows)] += A[np.ix_(cols[0], cols[0])]
        g[k0][rows] += b[cols[0]]
        return
    for kf, role in ((k0, 0), (k1, 1)):
        diag[kf][np.ix_(rows, rows)] += A[np.ix_(cols[role], cols[role])]
        g[kf][rows] += b[cols[role]]
    l = term["edge"] // 2
    ra, rb = (0, 1) if term["edge"] % 2 == 0 else (1, 0)      # link block: rows = older keyframe, columns = newer
    lnk[l][np.ix_(rows, rows)] += A[np.ix_(cols[ra], cols[rb])]


def assemble(K, links, CS, terms, results):
    """the packed layout [diag | link | g | tail] of these terms' results, summed in fp64"""
    B = 7 + CS
    parts = (np.zeros((K, B, B)), np.zeros((len(links), B, B)), np.zeros((K, B)), np.zeros(4))
    for t, r in zip(terms, results):
        place(parts, K, links, CS, t, r)
    return np.concatenate([p.reshape(-1) for p in parts])


# ---------------------------------------------------------------------------------------------- shared cases and bars
THETAS = (0.0, 1e-4, 1e-2, 1.0, 2.5)
CAP = dict(AtA=2e-5, Atb=2e-5, error=1e-5)      # the keypoint terms' bars (tests/test_gpu_window_keypoints.py): never above
FLOOR = 2e-6


def random_pose(rng, rot=0.5, trans=1.0):
    return np.concatenate([so3_exp(rng.normal(0.0, rot, 3)).ravel(), rng.normal(0.0, trans, 3)])


def pose_pair(rng, theta):
    """two unit-size poses whose relative rotation R1^T R0 has angle theta (exactly the identity for theta = 0: R0 = R1)"""
    p1 = random_pose(rng)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R1 = p1[:9].reshape(3, 3)
    R0 = R1 if theta == 0.0 else R1 @ so3_exp(theta * axis)
    return np.concatenate([R0.ravel(), rng.normal(0.0, 1.0, 3)]), p1


def off_target(rng, pose0, pose1, s0, s1, kind, off=0.05):
    """a target whose residuals are `off` long in translation, in rotation (before its weight) and in log-scale"""
    cur = relative_pose12(pose0, pose1)
    d = rng.normal(size=3); d *= off / np.linalg.norm(d)
    w = rng.normal(size=3); w *= off / np.linalg.norm(w)
    ts0 = s0 * 1.1
    tt = (cur[9:] / s0 + d) * ts0 if kind == "rel_pose_scale" else cur[9:] + d
    return np.concatenate([(so3_exp(w) @ cur[:9].reshape(3, 3)).ravel(), tt]), ts0, ts0 * (s1 / s0) * np.exp(off)


def binary_case(rng, theta, kind, s0=1.0, s1=1.0, on_target=False, weight=2.0, rot_weight=1.5, scale_weight=3.0, rounded=True):
    """-> (term without edge, pose0, pose1, s0, s1).  rounded: the poses are rounded to fp32, what the engine is given (the
    finite-difference check wants them orthonormal to fp64: on a matrix 6e-8 off the rotations the two branches of a
    logarithm differ by 1e-9, which a difference quotient over 2e-6 turns into 5e-4)"""
    p0, p1 = pose_pair(rng, theta)
    if rounded:
        p0, p1 = p0.astype(np.float32).astype(np.float64), p1.astype(np.float32).astype(np.float64)
    s0, s1 = float(np.float32(s0)), float(np.float32(s1))
    if on_target:
        tgt, ts0, ts1 = relative_pose12(p0, p1), s0, s1
    else:
        tgt, ts0, ts1 = off_target(rng, p0, p1, s0, s1, kind)
    term = dict(kind=kind, target_pose10=tgt.astype(np.float32), target_scale0=float(np.float32(ts0)),
                target_scale1=float(np.float32(ts1)), weight=weight, rot_weight=rot_weight, scale_weight=scale_weight)
    return term, p0, p1, s0, s1


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def fp32_distance(cases):
    """the fp32 restatement's own distance from the fp64 one over these (term, pose0, pose1, s0, s1): rel-L2 of the stacked
    AtA, of the stacked Atb and of the vector of errors"""
    l64 = [linearize(*c, dtype=np.float64) for c in cases]
    l32 = [linearize(*c, dtype=np.float32) for c in cases]
    return {k: rel_l2(np.concatenate([np.ravel(x[k]) for x in l32]), np.concatenate([np.ravel(x[k]) for x in l64]))
            for k in ("AtA", "Atb", "error")}


def parity_bars(cases):
    """4 x the fp32 restatement's distance over the same terms (the engine may round differently, it should not be another
    order), at least FLOOR, never above the keypoint terms' bars"""
    d = fp32_distance(cases)
    return {k: min(CAP[k], max(4.0 * d[k], FLOOR)) for k in d}, d


def on_target_bound(term):
    """seven residuals, each a rounding of a unit-size fp32 quantity"""
    return 1e-10 * term["weight"] * max(1.0, term.get("rot_weight", 1.0), term.get("scale_weight", 1.0))
