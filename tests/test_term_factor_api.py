"""The host definition of a window term's HessianFactor (sage_term_factor_block_count, sage_term_factor_blocks): the keys,
dims and columns a kind owns of its group's layout, the projection of its own sub-matrix in psd modes 0 / 1 / 2 and the cut
into upper blocks in push order -- against numpy selection + capi.nearest_psd / nearest_psd_reference + a cut written here.
No device."""
import os
import re

import numpy as np
import pytest

from sage_slam_amd import capi
from tests import psd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP, GRAPH = capi.TERM_KEYPOINT, capi.TERM_GRAPH
NEW = ("sage_term_factor_block_count", "sage_term_factor_blocks", "sage_window_keypoint_factor",
       "sage_window_keypoint_factor_error", "sage_window_graph_factor", "sage_window_graph_factor_error")


def shape(family, kind, CS):
    """the table of include/sage_ba.h -> (dims in push order, group D, first own column)"""
    if family == KP:
        return {0: ([6, 6, CS, 1], 13 + CS, 0), 1: ([6, 6, CS, CS, 1, 1], 14 + 2 * CS, 0), 2: ([6, 6, 1, 1], 14, 0)}[kind]
    return {0: ([6, 6, 1, 1], 14, 0), 1: ([6, 6], 14, 0), 2: ([1], 14, 12)}[kind]


KINDS = [(KP, 0), (KP, 1), (KP, 2), (GRAPH, 0), (GRAPH, 1), (GRAPH, 2)]


def expected(family, kind, CS, A, b, mode):
    dims, D, first = shape(family, kind, CS)
    Do = sum(dims)
    M = np.ascontiguousarray(A[first:first + Do, first:first + Do].astype(np.float64))
    Cm = M if mode == 0 else (capi.nearest_psd(M) if mode == 1 else capi.nearest_psd_reference(M))
    offs = np.concatenate([[0], np.cumsum(dims)])
    blocks = {(i, j): Cm[offs[i]:offs[i + 1], offs[j]:offs[j + 1]] for i in range(len(dims)) for j in range(i, len(dims))}
    g = b[first:first + Do].astype(np.float64)
    return blocks, [g[offs[i]:offs[i + 1]] for i in range(len(dims))], dims


def test_the_six_functions_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert re.search(r"SAGE_TERM_KEYPOINT\s*=\s*0\s*,\s*SAGE_TERM_GRAPH\s*=\s*1", hdr)


@pytest.mark.parametrize("CS", [16, 32])
def test_block_counts_are_the_tables_sums(CS):
    for family, kind in KINDS:
        dims = shape(family, kind, CS)[0]
        want = sum(dims[i] * dims[j] for i in range(len(dims)) for j in range(i, len(dims)))
        assert capi.term_factor_block_count(family, kind, CS) == want, (family, kind)
    # the two keypoint kinds that fill a dense layout count as the dense types do
    assert capi.term_factor_block_count(KP, 0, CS) == capi.lib().sage_factor_block_count(0, CS)
    assert capi.term_factor_block_count(KP, 1, CS) == capi.lib().sage_factor_block_count(1, CS)


def inputs(family, kind, CS):
    """the psd_ref families at the kind's group D; a sub-kind's non-zero entries confined to its own columns"""
    dims, D, first = shape(family, kind, CS)
    Do = sum(dims)
    for name in psd_ref.FAMILIES:
        for seed in range(2):
            A = np.zeros((D, D), np.float32)
            A[first:first + Do, first:first + Do] = psd_ref.family(name, Do, seed)
            r = np.random.default_rng([7, D, seed])
            b = np.zeros(D, np.float32)
            b[first:first + Do] = r.standard_normal(Do).astype(np.float32)
            yield name, seed, A, b


@pytest.mark.parametrize("family,kind,CS", [(KP, 2, 16), (GRAPH, 0, 16), (GRAPH, 1, 32), (GRAPH, 2, 16), (KP, 0, 32), (KP, 1, 32)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_blocks_are_selection_projection_and_cut_bit_for_bit(family, kind, CS, mode):
    dims_t, D, _ = shape(family, kind, CS)
    assert D in (14, 45, 78)
    for name, seed, A, b in inputs(family, kind, CS):
        blocks, gs, dims = capi.term_factor_blocks(family, kind, CS, A, b, mode)
        rb, rg, rdims = expected(family, kind, CS, A, b, mode)
        assert dims == rdims == dims_t
        assert sorted(blocks) == sorted(rb)
        for k in rb:
            assert blocks[k].shape == rb[k].shape and blocks[k].tobytes() == np.ascontiguousarray(rb[k]).tobytes(), (name, seed, k)
        assert len(gs) == len(rg) and all(a.tobytes() == c.tobytes() for a, c in zip(gs, rg)), (name, seed)


def test_the_full_layout_kinds_are_the_dense_types():
    """REPROJECTION = type 0 and MATCH_GEOMETRY = type 1: the same blocks as sage_factor_hessian_blocks, every mode"""
    for kind, CS in ((0, 16), (1, 16)):
        D = shape(KP, kind, CS)[1]
        A = psd_ref.family("gauge", D, 1); b = np.arange(D, dtype=np.float32)
        for mode in (0, 1, 2):
            blocks, gs, dims = capi.term_factor_blocks(KP, kind, CS, A, b, mode)
            rb, rg, rdims = capi.factor_hessian_blocks(kind, CS, A, b, mode)
            assert dims == rdims and all(blocks[k].tobytes() == rb[k].tobytes() for k in rb)
            assert all(a.tobytes() == c.tobytes() for a, c in zip(gs, rg))


@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("type_", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_dense_type_and_its_keypoint_kind_share_one_definition(CS, type_, mode):
    """what lets the dense factors and the terms share one path: on an indefinite (the projections do work), slightly
    asymmetric (the symmetrisation does work) system, sage_factor_hessian_blocks(type) and
    sage_term_factor_blocks(SAGE_TERM_KEYPOINT, kind = type) hand out the same bytes"""
    D = shape(KP, type_, CS)[1]
    r = np.random.default_rng([23, D])
    J = r.standard_normal((D // 2, D)).astype(np.float32)
    A = (J.T @ J - np.float32(0.3) * np.eye(D, dtype=np.float32)).astype(np.float32)
    A[1, D - 2] += np.float32(0.01)
    b = r.standard_normal(D).astype(np.float32)
    assert np.linalg.eigvalsh(psd_ref.symmetrised(A)).min() < 0 and not np.array_equal(A, A.T)
    blocks, gs, dims = capi.factor_hessian_blocks(type_, CS, A, b, mode)
    tb, tg, tdims = capi.term_factor_blocks(KP, type_, CS, A, b, mode)
    assert dims == tdims == shape(KP, type_, CS)[0]
    assert sorted(blocks) == sorted(tb)
    assert all(blocks[k].shape == tb[k].shape and blocks[k].tobytes() == tb[k].tobytes() for k in blocks)
    assert len(gs) == len(tg) and all(a.tobytes() == c.tobytes() for a, c in zip(gs, tg))


def test_a_sub_kind_ignores_the_columns_it_does_not_own():
    """REL_POSE projects its 12 x 12 and SCALE_PRIOR its 1 x 1 whatever stands in the rest of the 14 x 14"""
    r = np.random.default_rng(3)
    A = psd_ref.family("indefinite", 14, 0); b = r.standard_normal(14).astype(np.float32)
    for kind in (1, 2):
        dims, D, first = shape(GRAPH, kind, 16)
        Do = sum(dims)
        Z = np.zeros_like(A); Z[first:first + Do, first:first + Do] = A[first:first + Do, first:first + Do]
        for mode in (0, 1, 2):
            got = capi.term_factor_blocks(GRAPH, kind, 16, A, b, mode)
            ref = capi.term_factor_blocks(GRAPH, kind, 16, Z, b, mode)
            assert all(got[0][k].tobytes() == ref[0][k].tobytes() for k in ref[0])
            assert all(a.tobytes() == c.tobytes() for a, c in zip(got[1], ref[1]))
    # a negative scale-prior entry projects to zero
    A[12, 12] = np.float32(-2.0)
    assert capi.term_factor_blocks(GRAPH, 2, 16, A, b, 1)[0][(0, 0)].tolist() == [[0.0]]
    assert capi.term_factor_blocks(GRAPH, 2, 16, A, b, 0)[0][(0, 0)].tolist() == [[-2.0]]


def test_every_refusal():
    INVALID = -1
    for family, kind, CS in ((-1, 0, 16), (2, 0, 16), (KP, -1, 16), (KP, 3, 16), (GRAPH, -1, 16), (GRAPH, 3, 16), (KP, 0, 0),
                             (GRAPH, 1, -4)):
        assert capi.term_factor_block_count(family, kind, CS) == INVALID, (family, kind, CS)
    A = np.zeros((14, 14), np.float32); b = np.zeros(14, np.float32)
    G = np.zeros(14 * 14, np.float64); g = np.zeros(14, np.float64)
    ok = dict(family=GRAPH, kind=0, CS=16, AtA_ptr=A.ctypes.data, Atb_ptr=b.ctypes.data, psd_mode=1, G_ptr=G.ctypes.data,
              g_ptr=g.ctypes.data, dims_ptr=None, nkeys_ptr=None)
    assert capi.term_factor_blocks_raw(**ok) == 0                     # dims / nkeys are optional
    for bad in (dict(family=-1), dict(family=2), dict(kind=3), dict(kind=-1), dict(CS=0), dict(AtA_ptr=None), dict(Atb_ptr=None),
                dict(G_ptr=None), dict(g_ptr=None), dict(psd_mode=-1), dict(psd_mode=3)):
        assert capi.term_factor_blocks_raw(**{**ok, **bad}) == INVALID, bad
    with pytest.raises(capi.SageError) as ei:
        capi.term_factor_blocks(KP, 5, 16, A, b, 1)
    assert ei.value.code == INVALID
    # the window calls refuse a NULL window before anything else
    L = capi.lib()
    assert L.sage_window_keypoint_factor(None, 0, 1, None, None, None, None, None) == INVALID
    assert L.sage_window_graph_factor(None, 0, 1, None, None, None, None, None) == INVALID
    assert L.sage_window_keypoint_factor_error(None, 0, None) == INVALID
    assert L.sage_window_graph_factor_error(None, 0, None) == INVALID
