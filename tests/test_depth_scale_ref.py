"""The numpy restatement of the depth-scale correction (tests/depth_scale_ref.py) against the reference's own tensor
expressions on torch CPU tensors, the known answer of the synthetic pair, the lower median, the binding, and the seeds of
the GPU cases (tests/test_gpu_depth_scale.py).  No GPU.

What "the median is identical" means here: torch's grid_sample and matmul order a few fp64 operations differently from the
restatement, so per-point ratios agree to 1e-12 relative (about twenty fp64 roundings), not bit for bit.  The median is
therefore checked twice: ``lower_median`` of torch's OWN per-point ratios equals ``torch.median`` exactly (same element, NaN
propagation and the empty case included), and the restatement's median is within the per-point 1e-12 of torch's with the
same NaN-ness.  Measured: the two medians differ by at most one unit in the last place (2.2e-16 relative)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import depth_scale_ref as ref

# name -> (H, W, pose, seed, variant): the cases of tests/test_gpu_depth_scale.py.  The seeds are the first at which the
# fp64 restatement finds no ambiguous point (test_gpu_cases_have_no_ambiguous_point)
CASES = {
    "plain": (48, 64, "small", 1, "plain"),
    "zero_patch": (48, 64, "small", 1, "zero_patch"),
    "nan_texel": (48, 64, "small", 1, "nan_texel"),
    "behind": (48, 64, "behind", 0, "plain"),
    "plain96": (96, 128, "small", 16, "plain"),
    "big96": (96, 128, "big", 5, "plain"),
}
TRUE_SCALE = 1.7


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, fp64 points, fp32 points, number of ambiguous points): computed once, never changed"""
    H, W, pose, seed, variant = CASES[name]
    prob = synth.make_depth_scale_problem(H, W, pose, seed, TRUE_SCALE, variant)
    return prob, ref.points(prob, np.float64), ref.points(prob, np.float32), int(ref.ambiguous(prob).sum())


@pytest.mark.parametrize("name", ["plain", "zero_patch", "nan_texel", "behind"])
@pytest.mark.parametrize("drop_nan", [False, True])
def test_restatement_is_the_reference_expression(name, drop_nan):
    import torch
    prob, p64, _, _ = case(name)
    ratios, selected, med = ref.torch_expression(prob, torch.float64, drop_nan)
    assert np.array_equal(selected, p64["selected"])
    mine = p64["ratio"]
    assert np.array_equal(np.isnan(ratios), np.isnan(mine)) and np.array_equal(np.isinf(ratios), np.isinf(mine))
    fin = np.isfinite(mine) & (mine != 0)
    assert np.array_equal(ratios[~fin & ~np.isnan(mine)], mine[~fin & ~np.isnan(mine)])       # zeros and infinities, signs included
    rel = np.max(np.abs(ratios[fin] - mine[fin]) / np.abs(mine[fin])) if fin.any() else 0.0
    print(f"{name}: M {prob['M']} selected {int(selected.sum())} per-point rel {rel:.2e}")
    assert rel <= 1e-12
    # the median: the same function of the same values, exactly ...
    got, n_used, n_nan = ref.lower_median(ratios[selected], drop_nan)
    assert (np.isnan(got) and np.isnan(med)) or got == med
    # ... and the restatement's own within the per-point distance, NaN for NaN
    s = ref.stats(prob, np.float64, drop_nan, p64)
    assert (n_used, n_nan) == (s["n_used"], s["n_nan"])
    print(f"    median torch {med!r} restatement {s['ratio']!r} n_used {n_used} n_nan {n_nan}")
    assert np.isnan(s["ratio"]) == np.isnan(med)
    if not np.isnan(med):
        assert abs(s["ratio"] - med) <= 1e-12 * abs(med)
    if name == "behind":
        assert s["n_selected"] == 0 and np.isnan(med) and 0 < s["n_pos_depth"] < prob["M"]
    if name == "nan_texel":
        assert s["n_nan"] > 0 and np.isnan(med) == (not drop_nan)
    if name == "zero_patch":
        assert np.isinf(mine[selected]).sum() > 0 and np.isfinite(med)


@pytest.mark.parametrize("name", ["plain", "plain96", "big96"])
def test_known_answer(name):
    """the fp64 restatement recovers true_scale to within the spread of the per-point ratios (the scene's interpolation
    error: nothing the device code can change).  Measured |median - true| / IQR: plain 3.2e-3 / 6.3e-2, plain96 8.3e-3 /
    7.6e-2, big96 5.8e-3 / 7.0e-2"""
    prob, p64, _, _ = case(name)
    s = ref.stats(prob, np.float64, False, p64)
    r = p64["ratio"][p64["selected"]]
    p25, p75 = np.percentile(r, [25, 75])
    print(f"{name}: median {s['ratio']!r} true {prob['true_scale']} error {abs(s['ratio'] - prob['true_scale']):.3e} iqr {p75 - p25:.3e}")
    assert abs(s["ratio"] - prob["true_scale"]) <= p75 - p25


def test_lower_median():
    f = lambda *v: np.array(v, np.float32)
    med = lambda v, d=False: ref.lower_median(v, d)[0]
    assert med(f(3)) == 3 and med(f(2, 1)) == 1 and med(f(3, 1, 2)) == 2 and med(f(4, 1, 3, 2)) == 2
    assert med(f(5, 5, 5, 5)) == 5 and med(f(1, 2, 2, 3)) == 2 and med(f(1, 1, 2, 2)) == 1
    assert med(f(-0.0, 0.0)) == 0 and med(f(0.0, -0.0, -0.0)) == 0
    assert med(f(-np.inf, 1, np.inf)) == 1 and med(f(-np.inf, np.inf)) == -np.inf and med(f(np.inf, np.inf, 1)) == np.inf
    assert np.isnan(med(f(1, np.nan, 3))) and med(f(1, np.nan, 3), True) == 1
    assert ref.lower_median(f(1, np.nan, 3), True)[1:] == (2, 1) and ref.lower_median(f(1, np.nan, 3), False)[1:] == (3, 1)
    assert np.isnan(med(f())) and np.isnan(med(f(np.nan), True)) and ref.lower_median(f(np.nan), True)[1:] == (0, 1)
    import torch
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 9, 10):                                  # torch::median is this element
        v = rng.standard_normal(n).astype(np.float32)
        assert med(v) == torch.median(torch.from_numpy(v)).item()


def test_symbols_and_struct():
    from sage_slam_amd import capi
    L = capi.lib()
    assert L.sage_depth_scale_ratio is not None and L.sage_median_f32 is not None
    assert callable(capi.depth_scale_ratio) and callable(capi.median_f32)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sage_ba.h")).read()
    body = re.search(r"typedef struct SageDepthScaleStats\s*\{(.*?)\}\s*SageDepthScaleStats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(float|int32_t)\s+(\w+)\s*;", body)]
    assert [n for _, n in fields] == [n for n, _ in capi.SageDepthScaleStats._fields_]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert [ctype[t] for t, _ in fields] == [t for _, t in capi.SageDepthScaleStats._fields_]
    assert C.sizeof(capi.SageDepthScaleStats) == 4 * len(fields) == 24


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases_have_no_ambiguous_point(name):
    prob, p64, p32, n_amb = case(name)
    print(f"{name}: M {prob['M']} selected {int(p64['selected'].sum())} ambiguous {n_amb}")
    assert n_amb == 0
    assert np.array_equal(p64["selected"], p32["selected"]) and np.array_equal(p64["pos"], p32["pos"])
