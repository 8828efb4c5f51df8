"""Marginal priors on the host (include/sage_ba.h "f7"; no GPU): sage_schur_marginal against numpy's fp64 solve, Schur of
Schur, sage_prior_evaluate against the fp64 restatement of tests/marginal_ref.py, the layout plan of a window's prior terms,
and a stand-alone driver of marginal_host.cpp under AddressSanitizer and UBSan.

Bars.  The marginal: 64 n 2^-53 cond(A_dd) in relative Frobenius norm -- the textbook bound of a Cholesky solve, cond computed
here from the system under test; the systems are built with cond(A) = 1e5, and cond(A_dd) <= cond(A) <= 1e6 is asserted.
The term: both sides form Atb_i = eta_i - (Lambda delta)_i as a dot product of N = mB + 16 terms (16 for acos / sin /
the rotation product behind delta), each within gamma_N (|eta| + |Lambda||delta|)_i of the exact value, gamma_N = N 2^-53 /
(1 - N 2^-53): twice that between them."""
import os
import subprocess

import numpy as np
import pytest

from tests import marginal_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NOT_PSD = -1, -2, -3


@pytest.fixture(scope="module")
def capi():
    from sage_slam_amd import capi as c
    c.lib()
    return c


def random_spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return (Q * np.logspace(0.0, -np.log10(cond), n)) @ Q.T


def rel_fro(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def block_rows(blocks, B):
    return np.concatenate([np.arange(b * B, (b + 1) * B) for b in blocks])


SYSTEMS = [(3, 23), (4, 39)]


@pytest.fixture(scope="module")
def systems():
    out = {}
    for nb, B in SYSTEMS:
        rng = np.random.default_rng([nb, B])
        n = nb * B
        A = random_spd(rng, n, 1e5)
        A = A + 1e-9 * rng.normal(size=(n, n))             # not exactly symmetric: the call symmetrises on the way in
        out[(nb, B)] = (A, rng.normal(size=n), 1e3)
    return out


@pytest.mark.parametrize("nb,B", SYSTEMS)
@pytest.mark.parametrize("blocks", [(1,), (0, 2)])
def test_schur_marginal_against_numpy(capi, systems, nb, B, blocks):
    A, g, e = systems[(nb, B)]
    n = nb * B
    drop = block_rows(blocks, B)
    As = 0.5 * (A + A.T)
    cond = np.linalg.cond(As[np.ix_(drop, drop)])
    assert cond <= 1e6
    bar = 64.0 * n * 2.0 ** -53 * cond                    # the textbook bound, relative Frobenius norm
    Lam, eta, c = capi.schur_marginal(A, g, e, drop)
    LamR, etaR, cR = M.schur_marginal(A, g, e, drop)
    print(f"n={n} drop={blocks} cond(A_dd)={cond:.3e} bar={bar:.3e} Lambda {rel_fro(Lam, LamR):.3e} eta {rel_fro(eta, etaR):.3e} "
          f"c {abs(c - cR) / abs(cR):.3e}")
    assert rel_fro(Lam, LamR) <= bar
    assert rel_fro(eta, etaR) <= bar
    assert abs(c - cR) <= bar * abs(cR)
    assert np.array_equal(Lam, Lam.T)                      # symmetrised exactly


def test_schur_marginal_nonpositive_pivot_and_arguments(capi, systems):
    A, g, e = systems[(3, 23)]
    bad = A.copy()
    bad[23 + 3, 23 + 3] = -1.0
    rc, Lam, eta, c = capi.schur_marginal(bad, g, e, block_rows((1,), 23), check=False)
    assert rc == NOT_PSD                                   # the block solve's status for it
    assert np.isnan(Lam).all() and np.isnan(eta).all() and np.isnan(c)   # nothing written
    n = g.size
    assert capi.schur_marginal(A, g, e, [0, 0], check=False)[0] == INVALID          # a duplicate row
    assert capi.schur_marginal(A, g, e, [n], check=False)[0] == INVALID             # out of range
    assert capi.schur_marginal(A, g, e, np.arange(n), check=False)[0] == INVALID    # nothing to keep
    assert capi.schur_marginal_raw(None, g.ctypes.data, e, n, None, 0, None, None, None) == INVALID
    Lam, eta, c = capi.schur_marginal(A, g, e, [])         # nothing to drop: the symmetrised system itself
    assert np.array_equal(Lam, 0.5 * (A + A.T)) and np.array_equal(eta, g) and c == e


def test_identity_drop_rows_are_a_noop(capi, systems):
    """held variables of a dropped keyframe -- rows of the identity with a zero gradient (hold_packed's rule) -- eliminate to
    nothing: the same bits as the system without them"""
    A, g, e = systems[(4, 39)]
    B, n = 39, 4 * 39
    held = np.arange(B, B + 6)                             # the pose rows of block 1
    Ah, gh = A.copy(), g.copy()
    Ah[held, :] = 0.0; Ah[:, held] = 0.0; Ah[held, held] = 1.0; gh[held] = 0.0
    rest = np.setdiff1d(np.arange(n), held)
    drop_small = np.arange(B, 2 * B - 6)                   # the other rows of block 1 in the system without the held ones
    a = capi.schur_marginal(Ah, gh, e, block_rows((1,), B))
    b = capi.schur_marginal(Ah[np.ix_(rest, rest)], gh[rest], e, drop_small)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("nb,B", SYSTEMS)
def test_schur_of_schur(capi, systems, nb, B):
    A, g, e = systems[(nb, B)]
    n = nb * B
    L1, e1, c1 = capi.schur_marginal(A, g, e, block_rows((0,), B))
    L2, e2, c2 = capi.schur_marginal(L1, e1, c1, block_rows((0,), B))       # block 1 of A is block 0 of the result
    drop = block_rows((0, 1), B)
    L3, e3, c3 = capi.schur_marginal(A, g, e, drop)
    As = 0.5 * (A + A.T)
    bar = 64.0 * n * 2.0 ** -53 * np.linalg.cond(As[np.ix_(drop, drop)])
    print(f"n={n} bar={bar:.3e} Lambda {rel_fro(L2, L3):.3e} eta {rel_fro(e2, e3):.3e} c {abs(c2 - c3) / abs(c3):.3e}")
    assert rel_fro(L2, L3) <= bar and rel_fro(e2, e3) <= bar and abs(c2 - c3) <= bar * abs(c3)


# ------------------------------------------------------------------------------------------------------ the term
def so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def random_prior(rng, m, CS, angles=None):
    """a prior and variables whose rotations are angles[k] away from its linearisation point"""
    B = 7 + CS
    n = m * B
    Lam = random_spd(rng, n, 1e4) * 1e3
    x0 = [np.concatenate([so3_exp(rng.normal(size=3)).ravel(), rng.normal(size=3)]).astype(np.float32) for _ in range(m)]
    prior = dict(Lambda=0.5 * (Lam + Lam.T), eta=rng.normal(size=n) * 10.0, c=float(rng.uniform(1.0, 5.0)),
                 pose12=np.array(x0), code=rng.normal(0, 0.1, (m, CS)).astype(np.float32),
                 scale=rng.uniform(0.7, 1.4, m).astype(np.float32))
    angles = angles if angles is not None else np.exp(rng.uniform(np.log(1e-2), 0.0, m))
    pose = []
    for k in range(m):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        R = so3_exp(angles[k] * axis) @ x0[k][:9].reshape(3, 3).astype(np.float64)
        pose.append(np.concatenate([R.ravel(), x0[k][9:] + rng.normal(0, 0.05, 3)]).astype(np.float32))
    code = (prior["code"] + rng.normal(0, 0.02, (m, CS))).astype(np.float32)
    scale = (prior["scale"] * np.exp(rng.normal(0, 0.02, m))).astype(np.float32)
    return prior, np.array(pose), code, scale


@pytest.mark.parametrize("m,CS", [(1, 16), (3, 16), (4, 32), (16, 32)])
def test_prior_evaluate_against_restatement(capi, m, CS):
    rng = np.random.default_rng([m, CS])
    angles = np.exp(np.linspace(np.log(1e-2), 0.0, m))     # 1e-2 .. 1 rad: the logarithm's conditioning is not what is tested
    prior, pose, code, scale = random_prior(rng, m, CS, angles)
    P = capi.MarginalPrior(keyframes=np.arange(m) + 3, **prior)
    got = P.get()
    for key in ("Lambda", "eta", "pose12", "code", "scale"):
        assert np.array_equal(got[key], prior[key])
    assert got["c"] == prior["c"] and got["keyframes"].tolist() == list(range(3, m + 3)) and (P.m, P.CS) == (m, CS)
    out = P.evaluate(pose, code, scale)
    ref = M.prior_evaluate(prior, pose, code, scale)
    N = m * (7 + CS) + 16
    bA, bE = M.dot_bound(prior, ref["delta"], N)
    print(f"m={m} CS={CS} worst Atb {np.max(np.abs(out['Atb'] - ref['Atb']) / bA):.3f} of the bound, err "
          f"{abs(out['err'] - ref['err']) / bE:.3f}")
    assert np.allclose(out["delta"], ref["delta"], rtol=0, atol=16 * 2.0 ** -53 * np.max(np.abs(ref["delta"])) + 1e-300)
    assert np.all(np.abs(out["Atb"] - ref["Atb"]) <= 2.0 * bA)
    assert abs(out["err"] - ref["err"]) <= 2.0 * bE
    P.close()


def test_prior_handle_refusals(capi):
    rng = np.random.default_rng(3)
    prior, pose, code, scale = random_prior(rng, 2, 16)
    n = 2 * 23
    Lam, eta = prior["Lambda"], prior["eta"]
    h = capi.C.c_void_p()
    args = (Lam.ctypes.data, eta.ctypes.data, 0.0, prior["pose12"].ctypes.data, prior["code"].ctypes.data, prior["scale"].ctypes.data,
            None, capi.C.addressof(h))
    assert capi.marginal_prior_create_raw(0, 16, *args) == INVALID
    assert capi.marginal_prior_create_raw(17, 16, *args) == UNSUPPORTED       # the cap
    assert capi.marginal_prior_create_raw(2, 24, *args) == UNSUPPORTED        # a code size the engine does not instantiate
    assert capi.marginal_prior_create_raw(2, 16, None, *args[1:]) == INVALID
    assert capi.marginal_prior_create_raw(2, 16, *args[:-1], None) == INVALID
    assert capi.prior_evaluate_raw(None, pose.ctypes.data, code.ctypes.data, scale.ctypes.data, None, None, None) == INVALID
    P = capi.MarginalPrior(**prior)
    assert capi.prior_evaluate_raw(P.h, None, code.ctypes.data, scale.ctypes.data, None, None, None) == INVALID
    assert capi.prior_evaluate_raw(P.h, pose.ctypes.data, code.ctypes.data, scale.ctypes.data, None, None, None) == 0
    assert P.get()["keyframes"].tolist() == [0, 1] and n == P.m * P.B


# ------------------------------------------------------------------------------------------------------ the layout plan
def back_links(K, back=3):
    return [(i - d, i) for i in range(K) for d in range(1, back + 1) if i - d >= 0]


def test_plan_appends_missing_links_in_ascending_order(capi):
    K = 6
    links = back_links(K)                                  # (0,1) (0,2) (1,2) (0,3) ...: every pair at most 3 apart
    plan = capi.prior_term_plan(K, links, [[0, 1, 2, 5]])
    assert plan["append"] == [(0, 5), (1, 5)] == M.missing_links(links, [0, 1, 2, 5])
    # a second term sees the links the first one appended; its own come behind them, ascending
    plan = capi.prior_term_plan(K, links, [[5, 0], [4, 0, 5, 1]])
    assert plan["append"] == [(0, 5), (0, 4), (1, 5)]
    assert capi.prior_term_plan(K, links, [[2]])["append"] == []          # m = 1: no link block at all
    assert capi.prior_term_plan(K, links, [[2]])["place"] == [(0, 0, 0, 2, 0)]


def test_plan_placement_and_transposition(capi):
    K = 6
    links = back_links(K)
    kf_map = [4, 1, 3]                                     # not ascending: (4,1) and (4,3) sit in their link blocks transposed
    plan = capi.prior_term_plan(K, links, [kf_map])
    assert plan["append"] == []
    want = {}
    for i in range(3):
        want[(i, i)] = (kf_map[i], 0)
        for j in range(i + 1, 3):
            a, b = kf_map[i], kf_map[j]
            want[(i, j)] = (K + links.index((min(a, b), max(a, b))), int(a > b))
    got = {(i, j): (blk, tr) for _t, i, j, blk, tr in plan["place"]}
    assert got == want
    assert [p[3] for p in plan["place"]] == sorted(p[3] for p in plan["place"])    # block-major
    # the numbers behind it: the engine's placement, restated by place_prior on a random Lambda, is a symmetric system again
    rng = np.random.default_rng(0)
    CS, B = 16, 23
    Lam = random_spd(rng, 3 * B, 1e3)
    Lam = 0.5 * (Lam + Lam.T)
    packed = M.place_prior(K, links, CS, kf_map, Lam, rng.normal(size=3 * B), 1.0)
    H, _g, tail = capi.unpack_dense(packed, K, links, CS)
    idx = np.concatenate([np.arange(k * B, (k + 1) * B) for k in kf_map])
    assert np.array_equal(H[np.ix_(idx, idx)], Lam) and tail[1] == 1.0
    # two terms on one block: term-id order inside the block
    plan = capi.prior_term_plan(K, links, [[1, 2], [2, 1]])
    on_link = [p for p in plan["place"] if p[3] == K + links.index((1, 2))]
    assert on_link == [(0, 0, 1, K + links.index((1, 2)), 0), (1, 0, 1, K + links.index((1, 2)), 1)]


def test_plan_rank0_owns_every_term(capi):
    K, links = 5, back_links(5)
    for world in (1, 2, 4):
        for rank in range(world):
            plan = capi.prior_term_plan(K, links, [[0, 1], [3]], rank=rank, world=world)
            assert plan["owned"] == ([1, 1] if rank == 0 else [0, 0])
            assert (len(plan["place"]) > 0) == (rank == 0)
            assert plan["append"] == []                    # (the structure is every rank's)


def test_plan_refusals(capi):
    K, links = 20, back_links(20)
    assert capi.prior_term_plan(K, links, [list(range(17))], check=False)[0] == UNSUPPORTED   # m = 17
    assert capi.prior_term_plan(K, links, [list(range(16))], check=False)[0] == 0
    assert capi.prior_term_plan(K, links, [[1, 2, 1]], check=False)[0] == INVALID            # a duplicate id
    assert capi.prior_term_plan(K, links, [[1, K]], check=False)[0] == INVALID
    assert capi.prior_term_plan(K, links, [[-1]], check=False)[0] == INVALID
    assert capi.prior_term_plan(K, links, [[]], check=False)[0] == INVALID
    assert capi.prior_term_plan(K, links, [[0]], rank=2, world=2, check=False)[0] == INVALID


# ------------------------------------------------------------------------------------------------------ sanitizers
def test_standalone_driver_under_sanitizers(tmp_path):
    """integration/compile_check/marginal_check.cpp links marginal_host.cpp alone (no HIP, no engine library) and runs the
    first two cases above under AddressSanitizer and UBSan, on the CPU"""
    from sage_slam_amd import build as sage_build
    cxx = sage_build.HOSTCXX
    if not os.path.exists(cxx):
        pytest.fail(f"{cxx} is missing: the host compiler the library itself is built with")
    exe = str(tmp_path / "marginal_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sage_slam_amd", "csrc"),
                           os.path.join(ROOT, "integration", "compile_check", "marginal_check.cpp"),
                           os.path.join(ROOT, "sage_slam_amd", "csrc", "marginal_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "marginal_check ok" in r.stdout
