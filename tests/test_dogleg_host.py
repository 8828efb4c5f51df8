"""The dogleg's host code (csrc/dogleg_host.cpp; no device needed): the dogleg point, the trust-region iteration around a
callback in gtsam's three adaptation modes, the product kernels' incidence lists, argument checks and exports.

The references are tests/dogleg_ref.py (the iteration, restated from DoglegOptimizerImpl.h:137-252) and, for the point, the
vectors themselves: u = (g.g / g.Ag) g and n = A^-1 g of a seeded positive definite system, blended as
DoglegOptimizerImpl.cpp:25-83 blends them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import dogleg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NOT_PSD = 0, -1, -3
NEW = ("sage_dogleg_config_default", "sage_dogleg_point", "sage_dogleg_iterate", "sage_dogleg_incidence",
       "sage_window_dogleg_step", "sage_window_dogleg_run", "sage_window_dogleg_products", "sage_window_dogleg_candidate",
       "sage_window_get_dogleg_vectors")
MODES = (ref.SEARCH_EACH_ITERATION, ref.SEARCH_REDUCE_ONLY, ref.ONE_STEP_PER_ITERATION)


def system(seed, dim=6):
    """a seeded positive definite A with cond ~ 1e2, g, n = A^-1 g and their dots"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    A = Q @ np.diag(np.geomspace(1.0, 100.0, dim)) @ Q.T
    A = 0.5 * (A + A.T)
    g = rng.standard_normal(dim)
    n = np.linalg.solve(A, g)
    return A, g, n, ref.dots_of(A, g, n)


def close(a, b, tol=1e-12):
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) <= tol * max(abs(a), abs(b), 1e-300) or a == b


# ------------------------------------------------------------------------------------------------------------- declarations
def test_header_declares_and_library_exports():
    with open(os.path.join(ROOT, "include", "sage_ba.h")) as fh:
        hdr = fh.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^(int|void) " + name + r"\(", hdr, re.M), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    assert re.search(r"SAGE_DOGLEG_SEARCH_EACH_ITERATION = 0, SAGE_DOGLEG_SEARCH_REDUCE_ONLY = 1, "
                     r"SAGE_DOGLEG_ONE_STEP_PER_ITERATION = 2", hdr)
    cfg = capi.dogleg_config_default()
    assert (cfg.init_delta, cfg.min_delta, cfg.mode) == (1.0, 1e-5, capi.SAGE_DOGLEG_ONE_STEP_PER_ITERATION)
    assert C.sizeof(capi.SageDoglegState) == 15 * 8 + 5 * 4 + 4        # nine doubles and the dots, five ints, padded to 8
    assert C.sizeof(capi.SageDoglegConfig) == 24


# ------------------------------------------------------------------------------------------------------------------ the point
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_point_in_the_three_regions(seed):
    A, g, n, d = system(seed)
    u = d[ref.GG] / d[ref.GAG] * g
    nu, nn = np.linalg.norm(u), np.linalg.norm(n)
    assert nu < nn
    for delta, region in ((0.5 * nu, 0), (0.5 * (nu + nn), 1), (0.999 * nn, 1), (1.5 * nn, 2)):
        rc, a, b, reg = capi.dogleg_point(delta, d[ref.GG], d[ref.GN], d[ref.NN], d[ref.GAG])
        assert (rc, reg) == (OK, region)
        got = a * g + b * n
        if region == 0:
            want = delta * u / nu
        elif region == 2:
            want = n
            assert (a, b) == (0.0, 1.0)
        else:                                                          # the blend, from the vectors (ComputeBlend)
            un, uu, n2 = u @ n, u @ u, n @ n
            qa, qb, qc = uu - 2 * un + n2, 2 * (un - uu), uu - delta * delta
            roots = [(-qb + s * np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa) for s in (1, -1)]
            tau = [t for t in roots if 0 <= t <= 1][0]
            want = (1 - tau) * u + tau * n
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        if region < 2:
            assert abs(np.linalg.norm(got) - delta) <= 1e-12 * delta
        ra, rb, rreg = ref.point(delta, d[ref.GG], d[ref.GN], d[ref.NN], d[ref.GAG])
        assert close(a, ra) and close(b, rb) and reg == rreg


def test_point_at_the_boundaries_and_degenerate_inputs():
    # g.g = 4, g.Ag = 2: u = 2 g, |u|^2 = 16; u.n = 18, |n|^2 = 25
    assert capi.dogleg_point(3.0, 4.0, 9.0, 25.0, 2.0) == (OK, 1.5, 0.0, 0)        # inside: u scaled to 3 / 4
    assert capi.dogleg_point(4.0, 4.0, 9.0, 25.0, 2.0) == (OK, 2.0, 0.0, 1)        # delta^2 = |u|^2: the blend at tau = 0
    assert capi.dogleg_point(5.0, 4.0, 9.0, 25.0, 2.0) == (OK, 0.0, 1.0, 2)        # delta^2 = |n|^2: the Gauss-Newton point
    assert capi.dogleg_point(1.0, 0.0, 0.0, 0.0, 0.0) == (OK, 0.0, 0.0, 0)         # g = 0: converged, the zero step
    assert capi.dogleg_point(1.0, 0.0, 0.0, 0.0, -1.0) == (OK, 0.0, 0.0, 0)
    for gAg in (0.0, -1.0, float("nan")):
        assert capi.dogleg_point(1.0, 4.0, 9.0, 25.0, gAg)[0] == NOT_PSD
    f = capi.lib().sage_dogleg_point
    f.argtypes = [C.c_double] * 5 + [C.c_void_p] * 3
    x = C.c_double()
    r = C.c_int()
    for args in ((None, C.addressof(x), C.addressof(r)), (C.addressof(x), None, C.addressof(r)), (C.addressof(x), C.addressof(x), None)):
        assert f(1.0, 4.0, 9.0, 25.0, 2.0, *args) == INVALID


# -------------------------------------------------------------------------------------------------------------- the iteration
def run_both(mode, d, f_error, fn, delta0=None, min_delta=1e-5):
    """the engine's iteration and the restatement's over the same callback -> (state, reference dict, the two call lists)"""
    cfg = capi.dogleg_config_default()
    cfg.mode, cfg.min_delta = mode, min_delta
    st = capi.SageDoglegState()
    if delta0 is not None:
        st.delta = delta0
    calls, rcalls = [], []

    def rec(log):
        def f(a, b):
            log.append((a, b))
            return fn(a, b)
        return f

    rc = capi.dogleg_iterate(cfg, d, f_error, rec(calls), st)
    assert rc == OK
    want = ref.iterate(cfg.init_delta if delta0 is None else delta0, mode, d, f_error, rec(rcalls), min_delta)
    return st, want, calls, rcalls


def assert_same(st, want, calls, rcalls, d):
    for name in ("delta", "rho", "a", "b", "candidate_error"):
        assert close(getattr(st, name), want[name]), (name, getattr(st, name), want[name])
    assert (st.region, st.evals, st.accepted) == (want["region"], want["evals"], want["accepted"])
    assert len(calls) == len(rcalls) == st.evals
    for (a, b), (ra, rb) in zip(calls, rcalls):
        assert close(a, ra) and close(b, rb)
    assert close(st.step_norm, ref.step_norm(d, st.a, st.b))
    assert close(st.gn_norm, float(np.sqrt(d[ref.NN]))) and close(st.sd_norm, float(d[ref.GG] / d[ref.GAG] * np.sqrt(d[ref.GG])))
    assert np.array_equal(np.array(st.dots), np.asarray(d, np.float64))
    assert st.iters == 1 and st.solves == 0                            # (the window step counts the solves)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_iterate_on_a_quadratic(mode, seed):
    """the model is exact: rho = 1 in every evaluation, the radius only grows"""
    A, g, n, d = system(seed)
    E0 = 10.0

    def f(a, b):
        x = a * g + b * n
        return E0 - 2 * g @ x + x @ A @ x

    for delta0 in (None, 1e-2, 100.0):
        st, want, calls, rcalls = run_both(mode, d, E0, f, delta0)
        assert_same(st, want, calls, rcalls, d)
        assert abs(st.rho - 1.0) < 1e-9 and st.accepted == 1 and st.candidate_error < st.error == E0
        assert st.delta >= (delta0 or 1.0)
        assert st.evals == 1 if mode != ref.SEARCH_EACH_ITERATION else st.evals >= 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_iterate_on_a_quartic_that_overshoots(mode, seed):
    """a quartic term makes the Gauss-Newton point a bad one: the radius shrinks (and, searching, the point is re-evaluated)"""
    A, g, n, d = system(seed)
    E0, c = 10.0, 40.0 / float(n @ n) ** 2 * float(g @ n)

    def f(a, b):
        x = a * g + b * n
        return E0 - 2 * g @ x + x @ A @ x + c * float(x @ x) ** 2

    for delta0 in (None, 10.0 * float(np.linalg.norm(n))):
        st, want, calls, rcalls = run_both(mode, d, E0, f, delta0)
        assert_same(st, want, calls, rcalls, d)
    assert st.delta < 10.0 * float(np.linalg.norm(n)) and st.evals >= 1


@pytest.mark.parametrize("mode", MODES)
def test_iterate_on_a_function_that_rises_along_every_step(mode):
    """delta is halved from 1.0 until it is <= 1e-5 (17 times: 2^-17 = 7.6e-6), each radius evaluated once; then the zero step
    and the error kept"""
    A, g, n, d = system(5)
    E0 = 3.0

    def f(a, b):
        return E0 + float(np.linalg.norm(a * g + b * n))

    st, want, calls, rcalls = run_both(mode, d, E0, f)
    assert_same(st, want, calls, rcalls, d)
    assert st.evals == want["evals"] == 18
    assert st.delta == 2.0 ** -17 and (st.a, st.b, st.accepted, st.step_norm) == (0.0, 0.0, 0, 0.0)
    assert st.candidate_error == st.error == E0 and st.rho < 0


@pytest.mark.parametrize("mode", MODES)
def test_iterate_with_a_callback_that_returns_nan(mode):
    A, g, n, d = system(6)
    st, want, calls, rcalls = run_both(mode, d, 2.0, lambda a, b: float("nan"))
    assert_same(st, want, calls, rcalls, d)
    assert np.isnan(st.rho) and st.evals == 18 and st.accepted == 0 and st.candidate_error == st.error == 2.0
    # NaN only beyond a radius: the first finite evaluation decides
    st, want, calls, rcalls = run_both(mode, d, 2.0, lambda a, b: float("nan") if np.linalg.norm(a * g + b * n) > 0.1 else 1.9)
    assert_same(st, want, calls, rcalls, d)
    assert st.accepted == 1 and st.candidate_error == 1.9 and st.evals > 1


# A = I in one dimension, n = g, every dot 1: at delta 1 the point is n and the model decrease 1; at delta 0.5 it is g / 2
# and the model decrease 0.75 -- rho = -f / decrease is exact for f_error = 0
UNIT = np.ones(6)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("delta0,m_dec,step", [(1.0, 1.0, 1.0), (0.5, 0.75, 0.5)])
def test_iterate_at_the_thresholds_of_rho(mode, delta0, m_dec, step):
    assert ref.model_decrease(UNIT, *ref.point(delta0, 1, 1, 1, 1)[:2]) == m_dec
    for rho, grown in ((0.75, True), (0.25, False)):
        st, want, calls, rcalls = run_both(mode, UNIT, 0.0, lambda a, b: -rho * ref.model_decrease(UNIT, a, b), delta0)
        assert_same(st, want, calls, rcalls, UNIT)
        if mode == ref.ONE_STEP_PER_ITERATION:
            assert st.rho == rho and st.evals == 1 and st.accepted == 1 and st.step_norm == step
            assert st.delta == (max(delta0, 3.0 * step) if grown else delta0)
    # just below a threshold the other branch is taken: the radius is kept, then halved
    for rho, delta in ((np.nextafter(0.75, 0), delta0), (np.nextafter(0.25, 0), 0.5 * delta0)):
        st, want, calls, rcalls = run_both(ref.ONE_STEP_PER_ITERATION, UNIT, 0.0,
                                           lambda a, b: -rho * ref.model_decrease(UNIT, a, b), delta0)
        assert_same(st, want, calls, rcalls, UNIT)
        assert st.delta == delta and st.accepted == 1


@pytest.mark.parametrize("mode", MODES)
def test_iterate_at_rho_zero(mode):
    """An error that does not move at all is the 1e-15 rule's case (rho = 0.5), so rho = 0 itself is reached only from either
    side: a decrease of 1e-14 against a model decrease of 2e10 is the 0 <= rho < 0.25 branch (halve, take the step), the same
    increase the last branch (halve and evaluate again)."""
    st, want, calls, rcalls = run_both(mode, UNIT, 0.0, lambda a, b: 0.0)
    assert_same(st, want, calls, rcalls, UNIT)
    assert (st.rho, st.delta, st.evals, st.accepted) == (0.5, 1.0, 1, 1)
    big = UNIT * 1e20
    assert ref.model_decrease(big, *ref.point(1.0, *big[:4])[:2]) > 1e10
    st, want, calls, rcalls = run_both(mode, big, 0.0, lambda a, b: -1e-14)
    assert_same(st, want, calls, rcalls, big)
    assert 0.0 < st.rho < 1e-12 and st.accepted == 1
    if mode == ref.ONE_STEP_PER_ITERATION:
        assert (st.delta, st.evals) == (0.5, 1)
    st, want, calls, rcalls = run_both(mode, big, 0.0, lambda a, b: 1e-14)
    assert_same(st, want, calls, rcalls, big)
    assert -1e-12 < st.rho < 0.0 and st.accepted == 0 and st.evals == 18 and st.candidate_error == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_iterate_with_decreases_below_1e_15(mode):
    """either decrease below 1e-15 in magnitude: rho = 0.5, the radius is kept and the step taken"""
    A, g, n, d = system(7)
    for f_of in (lambda a, b: 5.0 - 1e-16, lambda a, b: 5.0, lambda a, b: 5.0 + 4e-16):
        st, want, calls, rcalls = run_both(mode, d, 5.0, f_of)
        assert_same(st, want, calls, rcalls, d)
        assert (st.rho, st.delta, st.evals, st.accepted) == (0.5, 1.0, 1, 1)
    tiny = d * 1e-17                                                   # the model's decrease below 1e-15
    st, want, calls, rcalls = run_both(mode, tiny, 5.0, lambda a, b: 4.0, 1e3)
    assert_same(st, want, calls, rcalls, tiny)
    assert (st.rho, st.delta, st.evals) == (0.5, 1e3, 1)


def test_iterate_vanishing_gradient_and_errors():
    cfg = capi.dogleg_config_default()
    st = capi.SageDoglegState()
    called = []
    assert capi.dogleg_iterate(cfg, np.zeros(6), 7.0, lambda a, b: called.append(1) or 0.0, st) == OK
    assert not called and (st.evals, st.accepted, st.iters, st.candidate_error, st.error, st.delta) == (0, 0, 1, 7.0, 7.0, 1.0)
    # g.Ag <= 0 and a failing callback: the code comes back, the state is untouched
    before = bytes(st)
    assert capi.dogleg_iterate(cfg, np.array([1, 1, 1, -1, 1, 1.0]), 7.0, lambda a, b: 0.0, st) == NOT_PSD

    def boom(a, b):
        raise RuntimeError("callback failure (expected by the test)")

    assert capi.dogleg_iterate(cfg, UNIT, 7.0, boom, st) == -4
    cfg.mode = 3
    assert capi.dogleg_iterate(cfg, UNIT, 7.0, lambda a, b: 0.0, st) == INVALID
    assert bytes(st) == before
    f = capi.lib().sage_dogleg_iterate
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, capi.DOGLEG_EVAL_FN, C.c_void_p, C.c_void_p]
    cb = capi.DOGLEG_EVAL_FN(lambda ctx, a, b, out: 0)
    cfg.mode = 2
    d = np.ones(6)
    null_cb = C.cast(None, capi.DOGLEG_EVAL_FN)
    assert f(None, d.ctypes.data, 1.0, cb, None, C.addressof(st)) == INVALID
    assert f(C.addressof(cfg), None, 1.0, cb, None, C.addressof(st)) == INVALID
    assert f(C.addressof(cfg), d.ctypes.data, 1.0, null_cb, None, C.addressof(st)) == INVALID
    assert f(C.addressof(cfg), d.ctypes.data, 1.0, cb, None, None) == INVALID


def test_state_carries_the_radius_across_iterations():
    A, g, n, d = system(8)
    cfg = capi.dogleg_config_default()
    st = capi.SageDoglegState()
    E0 = 1.0
    f = lambda a, b: E0 - 2 * g @ (a * g + b * n) + (a * g + b * n) @ A @ (a * g + b * n)
    assert capi.dogleg_iterate(cfg, d, E0, f, st) == OK
    first = st.delta
    want = ref.iterate(first, cfg.mode, d, E0, f)
    assert capi.dogleg_iterate(cfg, d, E0, f, st) == OK
    assert st.iters == 2 and close(st.delta, want["delta"]) and close(st.a, want["a"]) and close(st.b, want["b"])


# -------------------------------------------------------------------------------------------------------------- the incidence
def expected_incidence(K, links):
    lists = [[(k, 0)] for k in range(K)]
    for l, (a, b) in enumerate(links):
        lists[a].append((K + l, 0))
        lists[b].append((K + l, 1))
    off = np.cumsum([0] + [len(x) for x in lists])
    return off, np.array([e for x in lists for e in x], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("name,K,links", [
    ("chain", 5, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    ("hub of degree 9", 10, [(0, k) for k in range(1, 10)]),
    ("hub in the middle, ends either way round", 10, [(4, k) if k % 2 else (k, 4) for k in range(10) if k != 4]),
    ("duplicate link", 4, [(0, 1), (1, 2), (0, 1), (2, 3), (0, 1)]),
    ("two keyframes", 2, [(0, 1)]),
    ("no link", 3, []),
])
def test_incidence(name, K, links):
    rc, off, ent = capi.dogleg_incidence(K, links)
    woff, went = expected_incidence(K, links)
    assert rc == OK and np.array_equal(off, woff) and np.array_equal(ent, went)
    assert off[-1] == K + 2 * len(links)


def test_incidence_refuses_bad_arguments():
    assert capi.dogleg_incidence(0, [])[0] == INVALID
    for links in ([(0, 3)], [(-1, 1)], [(1, 1)], [(0, 1), (2, 5)]):
        assert capi.dogleg_incidence(3, links)[0] == INVALID
    f = capi.lib().sage_dogleg_incidence
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lk = np.array([[0, 1]], np.int32)
    off = np.zeros(3, np.int32)
    ent = np.zeros((4, 2), np.int32)
    assert f(2, 1, None, off.ctypes.data, ent.ctypes.data) == INVALID
    assert f(2, 1, lk.ctypes.data, None, ent.ctypes.data) == INVALID
    assert f(2, 1, lk.ctypes.data, off.ctypes.data, None) == INVALID
    assert f(2, -1, lk.ctypes.data, off.ctypes.data, ent.ctypes.data) == INVALID


def test_window_entry_points_refuse_null():
    L = capi.lib()
    st, cfg = capi.SageDoglegState(), capi.dogleg_config_default()
    d = np.zeros(6)
    cand = L.sage_window_dogleg_candidate
    cand.argtypes = [C.c_void_p, C.c_double, C.c_double]
    assert L.sage_window_dogleg_step(None, C.byref(st), C.byref(cfg)) == INVALID
    assert L.sage_window_dogleg_run(None, C.byref(st), C.byref(cfg), 1, None, None) == INVALID
    assert L.sage_window_dogleg_products(None, d.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert cand(None, 0.0, 1.0) == INVALID
    assert L.sage_window_get_dogleg_vectors(None, None, None, None, None) == INVALID
