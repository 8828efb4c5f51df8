"""The host half of the batched Higham projection (sage_factor_psd_batch and its window call): declarations and exports,
the plan's formulas, the Jacobi schedule the kernel walks, the argument checks that answer before anything touches a
device, and the host reference (sage_nearest_psd) pinned against a numpy restatement.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import psd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, OK = -1, 0
FUNCTIONS = ("sage_factor_psd_batch", "sage_factor_psd_batch_plan", "sage_jacobi_round_pairs",
             "sage_window_prepare_factors_device")


def test_header_declares_and_library_exports_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    L = capi.lib()
    for name in FUNCTIONS:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert re.search(r"#define\s+SAGE_PSD_MAX_DIM\s+80\b", hdr)
    m = re.search(r"typedef struct SagePsdStats\s*\{(.*?)\}\s*SagePsdStats;", hdr, re.S)
    assert m, "struct SagePsdStats"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.replace("\n", " ").split(";") if f.strip()]
    assert fields == ["int32_t status", "int32_t sweeps, bump_rounds", "double min_eig", "double off_norm"]
    assert C.sizeof(capi.SagePsdStats) == 32 and capi.SagePsdStats.min_eig.offset == 16
    assert capi.PSD_MAX_DIM == 80


@pytest.mark.parametrize("D", [1, 2, 29, 45, 46, 78, 80])
@pytest.mark.parametrize("n", [0, 1, 744])
def test_plan_equals_the_formulas_of_the_header(D, n):
    p = capi.factor_psd_batch_plan(D, n)
    Dc = (D + 15) // 16 * 16
    assert p["lds_bytes"] == 8 * (2 * Dc * (Dc | 1) + 4 * Dc + 64)
    assert p["device_bytes"] == 12 * n * D * D
    assert p["pinned_bytes"] == 32 * n
    assert p["launches"] == (2 if n else 0)
    assert p["lds_bytes"] <= 163840
    # the two matrices at the stride the kernel uses fit in what is declared
    assert 8 * 2 * D * (D | 1) <= p["lds_bytes"]


def test_plan_refuses_what_is_out_of_range():
    out = C.c_int64(7)
    for D, n in ((0, 1), (81, 1), (45, -1), (-3, 0)):
        assert capi.factor_psd_batch_plan_raw(D, n, C.addressof(out), None, None, None) == INVALID
    assert out.value == 7
    assert capi.factor_psd_batch_plan_raw(80, 744, None, None, None, None) == OK     # every output is optional
    assert capi.factor_psd_batch_plan(80, 1)["lds_bytes"] <= 163840


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 29, 45, 46, 78, 80])
def test_jacobi_schedule_visits_every_pair_once(D):
    rounds = D if D % 2 else D - 1
    seen = set()
    for r in range(rounds):
        pairs = capi.jacobi_round_pairs(D, r)
        assert len(pairs) == D // 2
        flat = [i for pq in pairs for i in pq]
        assert len(set(flat)) == len(flat), "pairs of a round are disjoint"
        assert all(0 <= p < q < D for p, q in pairs)
        assert not seen & set(pairs)
        seen |= set(pairs)
    assert len(seen) == D * (D - 1) // 2
    if D == 1:
        assert capi.jacobi_round_pairs(1, 0) == []
    buf = (C.c_int32 * 80)()
    for r in (-1, rounds, rounds + 1):
        assert capi.jacobi_round_pairs_raw(D, r, C.addressof(buf)) == INVALID
    assert capi.jacobi_round_pairs_raw(D, 0, None) == INVALID


def test_jacobi_schedule_refuses_a_dimension_out_of_range():
    buf = (C.c_int32 * 128)()
    for D in (0, -1, 81):
        assert capi.jacobi_round_pairs_raw(D, 0, C.addressof(buf)) == INVALID


def test_batch_argument_checks_answer_before_any_device_call():
    """Every refusal of sage_factor_psd_batch comes from the host check: with stand-in non-NULL pointers nothing may be
    dereferenced or launched (this machine may have no device at all)."""
    ws, a, c = C.c_void_p(64), C.c_void_p(64), C.c_void_p(64)   # never dereferenced by a refused call
    st = (capi.SagePsdStats * 1)()
    raw = capi.factor_psd_batch_raw
    assert raw(None, 45, 1, a, c, None) == INVALID
    assert raw(ws, 45, 1, None, c, None) == INVALID
    assert raw(ws, 45, 1, a, None, None) == INVALID
    assert raw(ws, 0, 1, a, c, None) == INVALID
    assert raw(ws, -1, 1, a, c, None) == INVALID
    assert raw(ws, 81, 1, a, c, None) == INVALID
    assert raw(ws, 45, -1, a, c, C.addressof(st)) == INVALID
    assert raw(None, 0, 0, None, None, None) == INVALID
    assert capi.factor_psd_batch_launches(None) == 0
    L = capi.lib()
    assert L.sage_window_prepare_factors_device(None, None) == INVALID
    f = L.sage_window_prepare_factors_device_launches
    f.argtypes = [C.c_void_p]
    assert f(None) == 0


def test_host_reference_agrees_with_the_numpy_restatement():
    """sage_nearest_psd against tests/psd_ref.py on the five input families, D in psd_ref.DIMS, six seeds each.
    Bar: ||difference||_F <= 1e-13 ||B||_F.  Measured on a CPU over all of them: worst 5.8e-15 (D = 78, indefinite, seed 2)
    with the draws of tests/psd_ref.py; 4.9e-15 (D = 45, indefinite) was measured on another draw of the same families when
    the bar was set.  The bar is a 17x to 20x margin over a measured value of the reference itself."""
    worst = (0.0, None)
    for D in psd_ref.DIMS:
        for name, seed, M in psd_ref.cases(D):
            M64 = M.astype(np.float64)
            got = capi.nearest_psd(M64)
            ref = psd_ref.nearest_psd(M64)
            nb = np.linalg.norm(psd_ref.symmetrised(M64))
            err = np.linalg.norm(got - ref)
            if nb > 0 and err / nb > worst[0]:
                worst = (err / nb, (D, name, seed))
            assert err <= 1e-13 * nb, (D, name, seed, err, nb)
            assert np.array_equal(got, got.T)
    print("worst ||sage_nearest_psd - psd_ref||_F / ||B||_F = %.3g at %s" % worst)
