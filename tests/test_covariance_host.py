"""Marginal covariances on the host (include/sage_ba.h "marginal covariances"): sage_block_covariance -- the selected inverse
of the block-envelope Cholesky factor -- against numpy.linalg.inv of the dense system (tests/covariance_ref.py), the symbolic
closure of the elimination plans, the refusals, and the argument checks of the window and depth-sigma entry points.  No GPU.

Bar: ||Sigma_hat - Sigma||_F <= 64 n 2^-53 cond_2(M) ||Sigma||_2 per block, n = K B; every case first asserts its own
precondition cond_2(M) <= 1e6 (the systems: J'J + I on the pattern with rows scaled over 1.5 decades, cond_2 1e2 .. 2e4).
Measured (printed by every run): the worst block lies 1e-7 .. 1e-5 of the bar."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import covariance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NOT_PSD, STATE = -1, -2, -3, -4
NEW = ["sage_block_covariance", "sage_covariance_plan", "sage_window_covariance", "sage_window_get_covariance",
       "sage_depth_sigma_batch", "sage_window_depth_sigma"]


@pytest.fixture(scope="module")
def capi():
    from sage_slam_amd import capi as c
    c.lib()
    return c


def back_links(K, back=3):
    return [(a, b) for b in range(K) for a in range(max(0, b - back), b)]


def random_system(K, B, links, seed):
    """J'J + I on the pattern: every link is a factor of 2B residual rows over its two keyframes -> diag [K,B,B],
    link blocks [n,B,B] (a link listed twice gets two factors)"""
    rng = np.random.default_rng(seed)
    diag = np.stack([np.eye(B) for _ in range(K)])
    blocks = []
    for a, b in links:
        Ja, Jb = (30.0 / np.sqrt(2 * B)) * rng.normal(size=(2, 2 * B, B))
        diag[a] += Ja.T @ Ja
        diag[b] += Jb.T @ Jb
        blocks.append(Ja.T @ Jb)
    d = 10.0 ** rng.uniform(-0.75, 0.75, (K, B))                     # rows of different units, as poses, codes and scales are
    diag = d[:, :, None] * diag * d[:, None, :]
    blocks = [d[a][:, None] * blk * d[b][None, :] for (a, b), blk in zip(links, blocks)]
    return diag, np.array(blocks).reshape(len(links), B, B)


def packed_of(K, B, diag, blocks):
    return np.concatenate([diag.reshape(-1), blocks.reshape(-1), np.zeros(K * B + 4)])


SHAPES = [
    ("K1", 1, 23, []),
    ("chain5-B7", 5, 7, back_links(5, 1)),
    ("chain5-B23", 5, 23, back_links(5, 1)),
    ("chain5-B39", 5, 39, back_links(5, 1)),
    ("K64-3back-B39", 64, 39, back_links(64)),
    ("K40-3back-loops-B23", 40, 23, back_links(40) + [(0, 39), (5, 30), (10, 20)]),
    ("duplicate-link", 5, 7, back_links(5, 1) + [(1, 2)]),
]
# blocks the closure of the recursion adds to the stored pattern of each plan: DESIGN.md s3 "Marginal covariances"
CLOSURE_ADDED = {"K1": 0, "chain5-B7": 0, "chain5-B23": 0, "chain5-B39": 0, "K64-3back-B39": 0, "K40-3back-loops-B23": 0,
                 "duplicate-link": 0}


@pytest.fixture(scope="module")
def systems():
    """per shape: diag, blocks (built once, shared by the cases)"""
    return {name: random_system(K, B, links, seed=7 + i) for i, (name, K, B, links) in enumerate(SHAPES)}


def test_header_and_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name
    assert "SAGE_DEPTH_VARIANCE = 0" in hdr and "SAGE_DEPTH_SIGMA = 1" in hdr and "typedef struct SageDepthSigmaItem" in hdr


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "diag_add"])
@pytest.mark.parametrize("damp", [0.0, 1e-3])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_block_covariance_against_the_dense_inverse(capi, systems, shape, damp, with_add):
    name, K, B, links = shape
    diag, blocks = systems[name]
    dadd = np.random.default_rng(3).uniform(0.0, 0.5, K * B) if with_add else None
    M = R.damped(R.dense_from_blocks(K, B, diag, links, blocks, dadd), damp)
    Sigma, cond, norm2 = R.covariance(M)
    assert cond <= 1e6, cond                                         # the test's own precondition
    uniq = sorted(set(links))
    pairs = [(k, k) for k in range(K)] + uniq + [(b, a) for a, b in uniq]
    packed = packed_of(K, B, diag, blocks)
    got = capi.block_covariance(packed, K, links, B, damp, pairs, dadd)
    bar = R.bar(K * B, cond, norm2)
    dist = [float(np.linalg.norm(got[i] - R.block(Sigma, B, a, b))) for i, (a, b) in enumerate(pairs)]
    print(f"{name} damp {damp:g} diag_add {with_add}: cond {cond:.3g}, worst block {max(dist):.3g}, bar {bar:.3g} "
          f"({max(dist) / bar:.2g} of it)")
    assert max(dist) <= bar
    for k in range(K):                                               # diagonal blocks: exactly symmetric
        assert np.array_equal(got[k], got[k].T)
    for i in range(len(uniq)):                                       # (b, a) is (a, b) transposed, bit for bit
        assert np.array_equal(got[K + len(uniq) + i], got[K + i].T)
    again = capi.block_covariance(packed, K, links, B, damp, pairs, dadd)
    assert again.tobytes() == got.tobytes()                          # run to run: the same bytes


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_closure_of_the_plans(capi, shape):
    name, K, _B, links = shape
    stored, added = capi.covariance_plan(K, links)
    print(f"{name}: the plan stores {stored} blocks, the closure adds {added}")
    assert stored >= K + len(set(links))
    assert added == CLOSURE_ADDED[name]


def test_refusals(capi, systems):
    name, K, B, links = SHAPES[1]
    diag, blocks = systems[name]
    packed = packed_of(K, B, diag, blocks)
    lk = np.ascontiguousarray(links, np.int32)

    def call(pk, K_, nl, B_, damp, pairs, out):
        pr = np.ascontiguousarray(pairs, np.int32)
        return capi.block_covariance_raw(pk.ctypes.data, K_, nl, lk.ctypes.data, B_, damp, None, pr.ctypes.data, len(pr), out.ctypes.data)

    out = np.full((2, B, B), 7.5)
    assert call(packed, K, len(links), B, 0.0, [(0, 0), (0, 2)], out) == INVALID and np.all(out == 7.5)   # not a link
    assert call(packed, K, len(links), B, 0.0, [(0, 0), (0, K)], out) == INVALID and np.all(out == 7.5)
    bad = packed.copy()
    bad[2 * B * B:3 * B * B] = -np.eye(B).reshape(-1)                 # keyframe 2: not positive definite
    assert call(bad, K, len(links), B, 0.0, [(0, 0), (0, 1)], out) == NOT_PSD and np.all(out == 7.5)       # the sentinel stays
    big = np.zeros(41 * 41 + 41 + 4); big[:41 * 41] = np.eye(41).reshape(-1)
    out41 = np.zeros((1, 41, 41))
    assert call(big, 1, 0, 41, 0.0, [(0, 0)], out41) == UNSUPPORTED
    f = capi.block_covariance_raw
    assert f(None, K, 0, None, B, 0.0, None, None, 0, None) == INVALID
    assert f(packed.ctypes.data, 0, 0, None, B, 0.0, None, None, 0, None) == INVALID
    assert f(packed.ctypes.data, K, 0, None, 0, 0.0, None, None, 0, None) == INVALID
    assert f(packed.ctypes.data, K, 1, None, B, 0.0, None, None, 0, None) == INVALID                       # links missing
    assert f(packed.ctypes.data, K, 0, None, B, 0.0, None, None, 1, out.ctypes.data) == INVALID            # pairs missing


def test_window_and_depth_entry_points_refuse_without_a_device(capi):
    """argument checks come before anything touches a window, a workspace or the device"""
    out = np.zeros(4)
    assert capi.window_covariance_raw(None, None) == INVALID
    assert capi.window_get_covariance_raw(None, 0, 0, out.ctypes.data) == INVALID
    assert capi.window_depth_sigma_raw(None, None, 0, 0, None) == INVALID
    fake = C.c_void_p(8)                                              # never dereferenced: the checks below come first
    table = (capi.SageDepthSigmaItem * 1)()
    addr = C.addressof(table)
    assert capi.depth_sigma_batch_raw(None, addr, 1, 2, 2, 16, 0) == INVALID
    assert capi.depth_sigma_batch_raw(fake, None, 1, 2, 2, 16, 0) == INVALID
    assert capi.depth_sigma_batch_raw(fake, addr, 0, 2, 2, 16, 0) == INVALID
    assert capi.depth_sigma_batch_raw(fake, addr, 1, 0, 2, 16, 0) == INVALID
    assert capi.depth_sigma_batch_raw(fake, addr, 1, 2, 2, 16, 2) == INVALID       # bad mode
    assert capi.depth_sigma_batch_raw(fake, addr, 1, 2, 2, 16, -1) == INVALID
    assert capi.depth_sigma_batch_raw(fake, addr, 1, 2, 2, 24, 0) == UNSUPPORTED   # bad CS
    assert capi.depth_sigma_batch_raw(fake, addr, 1, 2, 2, 32, 1) == INVALID       # an item of NULL arrays
