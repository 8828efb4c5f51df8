"""The gtsam glue EXECUTED for a window's terms: integration/compile_check/_bin/prepass_run with a terms file -- one term of
each of the six kinds on a K = 4 window -- hands every term through SageWindowCache::LinearizeTerm / ErrorTerm
(integration/sage_gtsam_prepass.h) into the recording gtsam::HessianFactor stand-in.  What arrives there is compared with
the table of include/sage_ba.h (keys in the reference's push order, dims) and, bit for bit, with what
Window.keypoint_factor / graph_factor hand out through ctypes at the same values, psd modes 0 and 1."""
import os
import struct
import subprocess

import numpy as np
import pytest

from sage_slam_amd import synth
from tests.test_gpu_gtsam_glue import BIN, _quat, _write_window
from tests.test_gpu_window_graph_terms import term_on_edge
from tests.test_gpu_window_keypoints import mg_term, rep_term
from tests.test_gpu_window_loop_graph import lmg_term

pytestmark = pytest.mark.gpu


def _write_terms(path, capi, kp, gt):
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(kp)))
        for t in kp:
            kind = capi.KP_KINDS[t["kind"]]
            N = np.asarray(t["homo0"]).shape[0]
            loss = capi.MG_LOSS[t["loss"]] if kind == capi.SAGE_KP_MATCH_GEOMETRY else 0
            f.write(struct.pack("<4i2f", kind, t["edge"], N, loss, t["loss_param"], t["weight"]))
            if kind == capi.SAGE_KP_REPROJECTION:
                f.write(i32(t["loc0"])); f.write(f32(t["homo0"])); f.write(f32(t["matched_2d"]))
            elif kind == capi.SAGE_KP_MATCH_GEOMETRY:
                f.write(i32(t["loc0"])); f.write(f32(t["homo0"])); f.write(i32(t["loc1"])); f.write(f32(t["homo1"]))
            else:
                f.write(f32(t["homo0"])); f.write(f32(t["homo1"])); f.write(f32(t["u0"])); f.write(f32(t["u1"]))
        f.write(struct.pack("<i", len(gt)))
        for t in gt:
            f.write(struct.pack("<3i", capi.GRAPH_KINDS[t["kind"]], t.get("edge", 0), t.get("kf", 0)))
            f.write(f32(t.get("target_pose10", np.zeros(12))))
            f.write(f32([t.get("target_scale0", 1.0), t.get("target_scale1", 1.0), t["weight"], t.get("rot_weight", 0.0),
                         t.get("scale_weight", 0.0)]))


def _read_records(raw, K, n):
    """the poses the Values hold, the recomputed count and n factor records (dense first, then the terms)"""
    o = 0
    poses = np.frombuffer(raw, np.float32, K * 12, o).reshape(K, 12).copy(); o += K * 48
    recomputed = struct.unpack_from("<i", raw, o)[0]; o += 4
    out = []
    for _ in range(n):
        nk = struct.unpack_from("<i", raw, o)[0]; o += 4
        keys = np.frombuffer(raw, np.uint64, nk, o).copy(); o += 8 * nk
        dims = np.frombuffer(raw, np.int32, nk, o).copy(); o += 4 * nk
        D = int(dims.sum())
        info = np.frombuffer(raw, np.float64, (D + 1) ** 2, o).reshape(D + 1, D + 1).copy(); o += 8 * (D + 1) ** 2
        err = struct.unpack_from("<d", raw, o)[0]; o += 8
        out.append(dict(keys=[int(k) for k in keys], dims=[int(d) for d in dims], info=info, error=err))
    assert o == len(raw)
    return poses, recomputed, out


@pytest.mark.skipif(not os.path.exists(BIN), reason="prepass_run is built in the build container (needs the reference's "
                                                    "vendored Eigen/Sophus) and travels with the tree")
@pytest.mark.parametrize("CS", [32, 16])
def test_gtsam_glue_delivers_every_term_kind(tmp_path, CS):
    import torch
    assert torch.cuda.is_available()
    from sage_slam_amd import capi
    w = synth.make_window(K=4, H=64, W=80, FS=16, CS=CS, L=4, seed=7, back_links=2)
    ne = 2 * len(w.links)
    rng = np.random.default_rng(3)
    kp = [rep_term(w, 0, n=40), mg_term(w, 3, "huber", n=33), lmg_term(w, w.links, 2, n=20)]
    gt = [term_on_edge(w, w.links, ne - 1, "rel_pose_scale", rng), term_on_edge(w, w.links, 1, "rel_pose", rng),
          dict(kind="scale_prior", kf=2, target_scale0=float(np.float32(w.keyframes[2].scale * 1.1)), weight=50.0)]
    values = []
    for k in w.keyframes:
        dR = synth.so3_exp(0.003 * rng.standard_normal(3))
        values.append((_quat(dR @ np.asarray(k.R, np.float64)), np.asarray(k.t, np.float32) + np.float32(0.003) * rng.standard_normal(3).astype(np.float32),
                       np.asarray(k.code, np.float32) + np.float32(0.01) * rng.standard_normal(CS).astype(np.float32),
                       np.float32(k.scale * (1 + 0.01 * rng.standard_normal()))))
    wb, tb, ob = str(tmp_path / "window.bin"), str(tmp_path / "terms.bin"), str(tmp_path / "out.bin")
    _write_window(wb, w, values)
    _write_terms(tb, capi, kp, gt)
    n_dense, n_terms = 2 * ne, len(kp) + len(gt)
    res = {}
    for psd in (0, 1):
        r = subprocess.run([BIN, wb, ob, str(psd), tb], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        res[psd] = _read_records(open(ob, "rb").read(), len(w.keyframes), n_dense + n_terms)
    poses, recomputed, _ = res[0]
    assert recomputed == 1
    win = capi.Window(w, keypoint_terms=kp, graph_terms=gt)
    codes = np.stack([v[2] for v in values]); scales = np.array([v[3] for v in values], np.float32)
    assert win.prepass(poses, codes, scales, jacobians=True)

    def kfs(e):
        a, b = w.links[e // 2]
        return (a, b) if e % 2 == 0 else (b, a)

    P, Cd, S = (lambda k: 1000 + k), (lambda k: 2000 + k), (lambda k: 3000 + k)
    expect = []
    for t in kp:
        k0, k1 = kfs(t["edge"])
        expect.append({"reprojection": ([P(k0), P(k1), Cd(k0), S(k0)], [6, 6, CS, 1]),
                       "match_geometry": ([P(k0), P(k1), Cd(k0), Cd(k1), S(k0), S(k1)], [6, 6, CS, CS, 1, 1]),
                       "loop_mg": ([P(k0), P(k1), S(k0), S(k1)], [6, 6, 1, 1])}[t["kind"]])
    for t in gt:
        if t["kind"] == "scale_prior":
            expect.append(([S(t["kf"])], [1]))
        else:
            k0, k1 = kfs(t["edge"])
            expect.append(([P(k0), P(k1), S(k0), S(k1)], [6, 6, 1, 1]) if t["kind"] == "rel_pose_scale" else ([P(k0), P(k1)], [6, 6]))
    for n, (keys, dims) in enumerate(expect):
        graph, i = n >= len(kp), n - len(kp) if n >= len(kp) else n
        for psd in (0, 1):
            got = res[psd][2][n_dense + n]
            assert got["keys"] == keys and got["dims"] == dims, (n, psd)
            info, D = got["info"], sum(dims)
            assert np.array_equal(info, info.T) and info[:D, :D].any()
            blocks, gs, f, sdims = win.graph_factor(i, psd) if graph else win.keypoint_factor(i, psd)
            assert sdims == dims
            offs = np.concatenate([[0], np.cumsum(dims)])
            for (a, b), blk in blocks.items():
                assert info[offs[a]:offs[a + 1], offs[b]:offs[b + 1]].tobytes() == blk.tobytes(), (n, psd, a, b)
            assert info[:D, D].tobytes() == np.concatenate(gs).tobytes() and info[D, D] == f and f > 0
            assert got["error"] == (win.graph_factor_error(i) if graph else win.keypoint_factor_error(i)) == f
    # the dense factors in front of them are the ones the window without a terms file hands out (tests/test_gpu_gtsam_glue.py)
    for t in (0, 1):
        for e in range(ne):
            got = res[1][2][t * ne + e]
            blocks, gs, f, dims = win.factor(t, e, psd_mode=1)
            offs = np.concatenate([[0], np.cumsum(dims)])
            assert got["dims"] == dims and got["info"][-1, -1] == f
            assert all(np.array_equal(got["info"][offs[a]:offs[a + 1], offs[b]:offs[b + 1]], blk) for (a, b), blk in blocks.items())
    win.close()
