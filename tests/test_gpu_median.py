"""sage_median_f32 (the exact radix selection of depth_scale.hip) against ``np.sort(x)[(n - 1) // 2]``: equal as floats, and
bit-identical except for the sign of a zero (the device orders -0 before +0, numpy's sort does not tell them apart).

Sizes: 1, 2, 3; 255, 256, 257 (one workgroup and its neighbour); 8191, 8192, 8193; 65536 and 65537 -- the grid of the key and
histogram kernels is capped at 256 workgroups of 256 threads, so 65537 values are more than one grid pass covers.  There is
no single-workgroup fast path, hence no further size limit to cross."""
import numpy as np
import pytest

from tests import depth_scale_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 65536, 65537]
F32 = np.float32


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


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same(got, want):
    """equal as floats, and the same bits unless both are zeros"""
    got, want = F32(got), F32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return bool(got == want) and (want == 0 or got.tobytes() == want.tobytes())


def check(capi, ws, x, drop_nan=False):
    x = np.asarray(x, F32)
    got, n_used, n_nan = capi.median_f32(ws, dev(x), None, drop_nan)
    want, want_used, want_nan = ref.lower_median(x, drop_nan)
    assert (n_used, n_nan) == (want_used, want_nan), (n_used, n_nan, want_used, want_nan)
    assert same(got, want), (got, want)
    return got


def contents(n, rng):
    """name -> n values"""
    half = np.arange(n) < (n + 1) // 2
    shared = (np.uint32(0x3fc00000) | rng.integers(0, 1 << 10, n).astype(np.uint32)).view(F32)   # one top-22-bit prefix
    ends = rng.standard_normal(n).astype(F32)
    ends[0] = -np.inf
    ends[-1] = np.inf
    out = {
        "normal": rng.standard_normal(n),
        "all_equal": np.full(n, 2.5),
        "two_values_50_50": rng.permutation(np.where(half, 1.0, 2.0)),
        "two_values_49_51": rng.permutation(np.where(np.arange(n) < (49 * n) // 100, 1.0, 2.0)),
        "shared_top_22_bits": shared,
        "negatives_and_positives": rng.standard_normal(n) * 1e3 - 100.0,
        "signed_zeros": rng.permutation(np.where(half, -0.0, 0.0)),
        "zeros_among_values": np.where(rng.random(n) < 0.5, rng.permutation(np.where(half, -0.0, 0.0)), rng.standard_normal(n)),
        "denormals": (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(F32),
        "inf_at_the_ends": ends,
        "all_inf": np.where(half, -np.inf, np.inf),
    }
    return {k: np.asarray(v, F32) for k, v in out.items()}


@pytest.mark.parametrize("n", SIZES)
def test_median_of_every_content(capi, ws, n):
    rng = np.random.default_rng([n, 77])
    for name, x in contents(n, rng).items():
        assert len(x) == n
        got = check(capi, ws, x)
        if n in (1, 257, 65537):
            print(f"n {n} {name}: {got!r}")


@pytest.mark.parametrize("n", [1, 2, 3, 257, 8193])
def test_a_nan_planted(capi, ws, n):
    """drop_nan 0: NaN, n_used = n; drop_nan 1: the median of the rest, n_used = n - n_nan (nothing left: NaN, n_used 0)"""
    rng = np.random.default_rng([n, 78])
    for k in sorted({1, min(n, 3), n}):               # one NaN, a few, and nothing but NaNs
        x = rng.standard_normal(n).astype(F32)
        x[rng.permutation(n)[:k]] = np.nan
        if k > 1:
            x[np.isnan(x).nonzero()[0][0]] = np.uint32(0xffc00001).view(F32)     # a NaN with the sign bit set
        got0 = check(capi, ws, x, False)
        got1 = check(capi, ws, x, True)
        assert np.isnan(got0) and np.isnan(got1) == (k == n)


def test_through_locations(capi, ws):
    """values[loc1d]: repeated and out-of-order indices into a larger map"""
    rng = np.random.default_rng(79)
    values = rng.standard_normal(5000).astype(F32)
    for n in (1, 300, 9000):
        loc = rng.integers(0, 5000, n).astype(np.int64)
        loc[: n // 3] = loc[0]                         # one index a third of the time
        got, n_used, n_nan = capi.median_f32(ws, dev(values), dev(loc))
        want = np.sort(values[loc])[(n - 1) // 2]
        assert (n_used, n_nan) == (n, 0) and same(got, want)
        assert capi.median_f32(ws, dev(values[loc]))[0].tobytes() == got.tobytes()


def test_two_calls_and_a_fresh_workspace_return_the_same_bytes(capi, ws):
    x = contents(8193, np.random.default_rng(80))["zeros_among_values"]
    a, b = capi.median_f32(ws, dev(x)), capi.median_f32(ws, dev(x))
    w2 = capi.Workspace()
    try:
        c = capi.median_f32(w2, dev(x))
    finally:
        w2.close()
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1:] == b[1:] == c[1:]


def test_misuse(capi, ws):
    import ctypes as C
    x = dev(np.arange(5, dtype=F32))
    med = C.c_float(-1.0)
    p = capi.dptr(x)
    assert capi.median_f32_raw(None, p, None, 5, 0, C.addressof(med), None, None) == -1
    assert capi.median_f32_raw(ws.h, None, None, 5, 0, C.addressof(med), None, None) == -1
    assert capi.median_f32_raw(ws.h, p, None, 5, 0, None, None, None) == -1
    assert capi.median_f32_raw(ws.h, p, None, 0, 0, C.addressof(med), None, None) == -1
    assert capi.median_f32_raw(ws.h, p, None, -3, 0, C.addressof(med), None, None) == -1
    assert med.value == -1.0
    assert capi.median_f32_raw(ws.h, p, None, 5, 0, C.addressof(med), None, None) == 0 and med.value == 2.0   # counts optional
    assert capi.median_f32(ws, x) == (F32(2.0), 5, 0)
