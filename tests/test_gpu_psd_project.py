"""The batched Higham projection on the device (sage_factor_psd_batch, sage_window_prepare_factors_device) against the
host's sage_nearest_psd, on the input families of tests/psd_ref.py.

Bar 1 (parity): ||C_dev - sage_nearest_psd(M)||_F <= 32 D 2^-52 ||B||_F.  Derived, not measured: a Jacobi eigensolver that
stops at off <= 2^-52 diag is backward stable to a small multiple of D eps ||B||_F per sweep, the projection onto the PSD
cone is 1-Lipschitz in the Frobenius norm, a bump moves the diagonal by a few ulps of its largest entry per round; the
factor 32 covers the sweep cap, the bumps and the reference's own 6e-15 (tests/test_psd_project_api.py).
Bar 3 (smallest eigenvalue): >= -D^2 2^-52 ||C_dev||_F, the backward-error bound of an unpivoted LDL^T that ended with
non-negative pivots."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import psd_ref

pytestmark = pytest.mark.gpu

EPS = psd_ref.EPS
SWEEP_CAP = 30


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


def project(capi, ws, mats):
    """[n, D, D] float32 numpy -> (C [n, D, D] float64 numpy, stats list)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(mats, np.float32)).cuda()
    out, stats = capi.factor_psd_batch(ws, t)
    return out.cpu().numpy(), stats


def stats_bytes(st):
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


_results = {}


@pytest.fixture(scope="module")
def projected(capi, ws):
    """per D, computed once: the cases, the device's results and the host reference's"""
    def get(D):
        if D not in _results:
            cases = psd_ref.cases(D)
            mats = np.stack([M for _, _, M in cases])
            Cd, stats = project(capi, ws, mats)
            assert capi.factor_psd_batch_launches(ws) == 2
            ref = np.stack([capi.nearest_psd(M.astype(np.float64)) for M in mats])
            _results[D] = (cases, mats, Cd, stats, ref)
        return _results[D]
    return get


def bar1(D, M):
    return 32 * D * EPS * np.linalg.norm(psd_ref.symmetrised(M))


@pytest.mark.parametrize("D", psd_ref.DIMS)
def test_parity_with_the_host(projected, D):
    cases, mats, Cd, stats, ref = projected(D)
    worst = {}
    for i, (name, seed, M) in enumerate(cases):
        err, bar = np.linalg.norm(Cd[i] - ref[i]), bar1(D, M)
        worst[name] = max(worst.get(name, 0.0), err / bar if bar > 0 else float(err > 0))
    print("D %d: worst ||C_dev - host||_F / bar per family: %s" % (D, ", ".join("%s %.3g" % kv for kv in worst.items())))
    for i, (name, seed, M) in enumerate(cases):
        assert np.linalg.norm(Cd[i] - ref[i]) <= bar1(D, M), (name, seed)


@pytest.mark.parametrize("D", psd_ref.DIMS)
def test_result_is_symmetric_bit_for_bit(projected, D):
    _, _, Cd, _, _ = projected(D)
    assert np.array_equal(Cd, np.transpose(Cd, (0, 2, 1)))


@pytest.mark.parametrize("D", psd_ref.DIMS)
def test_smallest_eigenvalue(projected, D):
    cases, _, Cd, _, _ = projected(D)
    for i, (name, seed, _) in enumerate(cases):
        ev = np.linalg.eigvalsh(Cd[i]).min()
        assert ev >= -D * D * EPS * np.linalg.norm(Cd[i]), (name, seed, ev)


@pytest.mark.parametrize("D", psd_ref.DIMS)
def test_stats(projected, D):
    cases, mats, Cd, stats, _ = projected(D)
    for i, (name, seed, M) in enumerate(cases):
        st = stats[i]
        assert st.status == 0, (name, seed)
        assert 0 <= st.sweeps < SWEEP_CAP and 0 <= st.bump_rounds <= 60, (name, seed, st.sweeps, st.bump_rounds)
        w = np.linalg.eigvalsh(psd_ref.symmetrised(M))
        scale = max(np.abs(w).max(), 1e-300)
        assert abs(st.min_eig - w.min()) <= 32 * D * EPS * scale * np.sqrt(D), (name, seed)
        assert st.off_norm <= 1.001 * EPS * np.linalg.norm(w)
        if name == "zeros":
            assert st.sweeps == 0 and st.bump_rounds == 0 and not Cd[i].any()
        if D == 1 and st.bump_rounds == 0:
            assert Cd[i][0, 0] == max(float(M[0, 0]), 0.0)
    print("D %d: most sweeps %d, most bump rounds %d" % (D, max(s.sweeps for s in stats), max(s.bump_rounds for s in stats)))
    if D == 1:
        # ... and with the bump rule: a bump is max(1e-15, one ulp of the entry) per round, doubling never reaches here
        for i, (name, seed, M) in enumerate(cases):
            m = max(float(M[0, 0]), 0.0)
            assert m <= Cd[i][0, 0] <= m + stats[i].bump_rounds * max(2e-15, 4 * EPS * m)


def mixed_45(n):
    names = psd_ref.FAMILIES
    return np.stack([psd_ref.family(names[i % len(names)], 45, 100 + i) for i in range(n)])


def test_a_result_does_not_depend_on_the_batch(capi, ws):
    mats = mixed_45(37)
    Cb, sb = project(capi, ws, mats)
    for i in range(37):
        C1, s1 = project(capi, ws, mats[i:i + 1])
        assert C1[0].tobytes() == Cb[i].tobytes(), i
        assert stats_bytes(s1[0]) == stats_bytes(sb[i]), i
    Cr, sr = project(capi, ws, mats[::-1])
    for i in range(37):
        assert Cr[36 - i].tobytes() == Cb[i].tobytes(), i
        assert stats_bytes(sr[36 - i]) == stats_bytes(sb[i]), i


def test_non_finite_input_is_reported_and_left_alone(capi, ws):
    good = mixed_45(9)
    Cg, sg = project(capi, ws, good)
    nan = psd_ref.family("indefinite", 45, 7).copy(); nan[3, 17] = np.nan
    inf = psd_ref.family("gauge", 45, 7).copy(); inf[44, 0] = np.inf; inf[2, 2] = -np.inf
    mats = np.concatenate([good[:4], nan[None], good[4:7], inf[None], good[7:]])
    Cm, sm = project(capi, ws, mats)          # (returns SAGE_OK: project raises otherwise)
    keep = [0, 1, 2, 3, 5, 6, 7, 9, 10]
    for j, i in enumerate(keep):
        assert Cm[i].tobytes() == Cg[j].tobytes() and stats_bytes(sm[i]) == stats_bytes(sg[j]), (i, j)
    for i, M in ((4, nan), (8, inf)):
        assert sm[i].status == 2 and sm[i].sweeps == 0 and sm[i].bump_rounds == 0
        with np.errstate(invalid="ignore"):
            want = psd_ref.symmetrised(M)
        assert np.array_equal(Cm[i], want, equal_nan=True)


def test_an_empty_batch_launches_nothing(capi, ws):
    import torch
    out, stats = capi.factor_psd_batch(ws, torch.empty((0, 45, 45), dtype=torch.float32, device="cuda"))
    assert out.shape == (0, 45, 45) and stats == [] and capi.factor_psd_batch_launches(ws) == 0


# ------------------------------------------------------------------------------------------------ the window path
def window_values(w):
    poses = np.stack([np.concatenate([np.asarray(k.R, np.float32).reshape(-1), np.asarray(k.t, np.float32).reshape(-1)])
                      for k in w.keyframes])
    codes = np.stack([np.asarray(k.code, np.float32).reshape(-1) for k in w.keyframes])
    scales = np.array([k.scale for k in w.keyframes], np.float32)
    return poses, codes, scales


def edges_now(win, ne):
    """the device's per-edge systems as they stand: right after a prepass, what the cache holds"""
    return {(t, e): win.get_edge(t, e) for t in (0, 1) for e in range(ne)}


def assert_serves(capi, win, CS, edges):
    """every block sage_window_factor(.., 1, ..) hands out against sage_factor_hessian_blocks(.., 1, ..) on `edges`: the
    blocks within bar 1 (over all blocks of the factor at once), g and f byte for byte"""
    for (t, e), he in edges.items():
        D = he["AtA"].shape[0]
        blocks, gs, f, dims = win.factor(t, e, psd_mode=1)
        rb, rg, rdims = capi.factor_hessian_blocks(t, CS, he["AtA"], he["Atb"], psd_mode=1)
        assert dims == rdims
        err = np.sqrt(sum(np.sum((blocks[k] - rb[k]) ** 2) for k in rb))
        assert err <= bar1(D, he["AtA"]), (t, e, err)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(gs, rg))
        assert f == he["error"]


@pytest.mark.parametrize("CS", [16, 32])
def test_window_prepares_its_factors_on_the_device(capi, CS):
    w = synth.make_window(K=4, H=64, W=80, FS=16, CS=CS, L=4, seed=11, back_links=3)
    assert len(w.links) == 6
    ne = 12
    win = capi.Window(w)
    with pytest.raises(capi.SageError) as ei:      # before any prepass
        win.prepare_factors_device()
    assert ei.value.code == -4
    poses, codes, scales = window_values(w)
    assert win.prepass(poses, codes, scales, jacobians=True)
    edges = edges_now(win, ne)
    worst = win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 2        # one per factor type
    assert worst.status == 0 and 0 < worst.sweeps < SWEEP_CAP
    assert_serves(capi, win, CS, edges)
    # the prepared matrices are what is served: the lazy path on the same input differs in the last bits
    again = win.prepare_factors_device()                     # prepared already: nothing launched
    assert win.prepare_factors_device_launches() == 0
    assert stats_bytes(again) == stats_bytes(worst)
    first = {k: win.factor(*k, psd_mode=1)[0] for k in edges}
    # host mode 2 afterwards replaces the device result and serves mode 2 as before
    win.prepare_factors(2, 0)
    for (t, e), he in edges.items():
        b2 = win.factor(t, e, psd_mode=2)[0]
        r2 = capi.factor_hessian_blocks(t, CS, he["AtA"], he["Atb"], psd_mode=2)[0]
        assert all(np.array_equal(b2[k], r2[k]) for k in r2)
    win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 2
    for k in edges:
        b = win.factor(*k, psd_mode=1)[0]
        assert all(b[j].tobytes() == first[k][j].tobytes() for j in b)
    # a recomputing prepass drops the preparation; the new values are served
    poses2 = poses.copy(); poses2[1, 9:] += np.float32(0.003)
    assert win.prepass(poses2, codes, scales, jacobians=True)
    edges2 = edges_now(win, ne)
    assert any(not np.array_equal(edges2[k]["AtA"], edges[k]["AtA"]) for k in edges)
    for (t, e), he in list(edges2.items())[:2]:              # not prepared: the lazy host path, bit for bit
        b = win.factor(t, e, psd_mode=1)[0]
        r = capi.factor_hessian_blocks(t, CS, he["AtA"], he["Atb"], psd_mode=1)[0]
        assert all(np.array_equal(b[k], r[k]) for k in r)
    win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 2
    assert_serves(capi, win, CS, edges2)
    win.close()


def test_window_uploads_the_cache_when_the_device_has_moved_on(capi):
    CS = 16
    w = synth.make_window(K=4, H=64, W=80, FS=16, CS=CS, L=4, seed=12, back_links=3)
    win = capi.Window(w)
    poses, codes, scales = window_values(w)
    assert win.prepass(poses, codes, scales, jacobians=True)
    edges_x = edges_now(win, 12)
    # other values and a linearize of the window's own: the device's per-edge systems are no longer those of X
    pose1, code1, s1 = win.get_keyframe(1)
    pose1 = pose1.copy(); pose1[9:] += np.float32(0.004)
    win.set_keyframe(1, pose1, code1 * np.float32(1.05), s1)
    win.linearize()
    edges_y = edges_now(win, 12)
    assert sum(not np.array_equal(edges_y[k]["AtA"], edges_x[k]["AtA"]) for k in edges_x) >= 12   # the edges at keyframe 1
    win.prepare_factors_device()
    assert win.prepare_factors_device_launches() == 2
    assert_serves(capi, win, CS, edges_x)
    win.close()
