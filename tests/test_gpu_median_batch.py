"""sage_median_f32_batch: element b against ``depth_scale_ref.lower_median`` (equal as floats and bit-identical except for the
sign of a zero, as in tests/test_gpu_median.py) and against sage_median_f32 on the same segment, byte for byte.

Segments of n = 1, 2, 3, 256, 257 and 4099 values (one workgroup, its neighbour, seventeen), side by side in one batch,
with and without locations, with both drop_nan settings.  Contents: normal values, all equal, signed zeros, infinities,
nothing but NaNs, and for each of the selection's three digits (11 + 11 + 10 bits of the order-preserving key) values that
differ in that digit only, with the wanted rank in its first and in its last bin.  The first digit's outermost bins that a
value can reach are those of -inf and +inf: the bins beyond hold only NaN patterns, which take no part."""
import numpy as np
import pytest

from tests import depth_scale_ref as ref
from tests.test_gpu_median import same

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 2, 3, 256, 257, 4099)


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


def from_keys(keys):
    """the floats whose order-preserving keys these are"""
    k = np.asarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def majority(pool, winner, n, rng):
    """n values of `pool` of which more than half are `winner`: the wanted rank lies on it"""
    x = rng.choice(pool, n)
    x[: n // 2 + 1] = winner
    return rng.permutation(x)


def digit_segments(n, rng):
    """per digit, the rank in the first and in the last bin"""
    base = np.uint32(0xbfc00000)                                             # the key of 1.5: a positive value
    low = from_keys(base | np.arange(1 << 10, dtype=np.uint32))              # differ in the low 10 bits only
    mid = from_keys(base | (np.arange(1 << 11, dtype=np.uint32) << 10))      # in the middle 11 bits only (the top 2 of `base`'s are 0)
    top_bits = np.concatenate([np.arange(0, 0x3fd, dtype=np.uint32), np.uint32(0x400) | np.arange(0, 0x3fd, dtype=np.uint32)]) << 21
    top = top_bits.view(F32)                                                 # in the top 11 bits only: -inf ... +inf, no NaN
    assert not np.isnan(top).any() and np.isinf(top).sum() == 2
    out = {}
    for name, pool in (("low", low), ("mid", mid), ("top", top)):
        s = np.sort(pool)
        out[name + "_first_bin"] = majority(pool, s[0], n, rng)
        out[name + "_last_bin"] = majority(pool, s[-1], n, rng)
        out[name + "_spread"] = rng.choice(pool, n)
    return out


def segments():
    """name -> values: every content at every size"""
    out = {}
    for n in SIZES:
        rng = np.random.default_rng([n, 91])
        half = np.arange(n) < (n + 1) // 2
        ends = rng.standard_normal(n).astype(F32)
        ends[0], ends[-1] = -np.inf, np.inf
        seg = {"normal": rng.standard_normal(n), "all_equal": np.full(n, 2.5), "signed_zeros": rng.permutation(np.where(half, -0.0, 0.0)),
               "inf_at_the_ends": ends, "all_inf": rng.permutation(np.where(half, -np.inf, np.inf)), "only_nans": np.full(n, np.nan),
               "a_nan": np.where(np.arange(n) == n // 2, np.nan, rng.standard_normal(n))}
        seg.update(digit_segments(n, rng))
        out.update({f"{k}_{n}": np.asarray(v, F32) for k, v in seg.items()})
    return out


def run_and_check(capi, ws, names, segs, drop_nan, with_loc):
    """one batch over the named segments; with_loc[b]: the segment is read through shuffled locations into a padded array"""
    rng = np.random.default_rng(92)
    values, locs, want_x = [], [], []
    for name, wl in zip(names, with_loc):
        x = segs[name]
        if wl:
            padded = np.concatenate([rng.standard_normal(5).astype(F32), x, rng.standard_normal(7).astype(F32)])
            loc = (5 + rng.permutation(len(x))).astype(np.int64)
            values.append(dev(padded)); locs.append(dev(loc)); want_x.append(padded[loc])
        else:
            values.append(dev(x)); locs.append(None); want_x.append(x)
    got = capi.median_f32_batch(ws, values, locs if any(with_loc) else None, drop_nan)
    assert len(got) == len(names) and capi.depth_scale_ratio_batch_launches(ws) == 5
    for name, g, x, v, l in zip(names, got, want_x, values, locs):
        want, n_used, n_nan = ref.lower_median(x, drop_nan)
        assert (g[1], g[2]) == (n_used, n_nan), (name, g, n_used, n_nan)
        assert same(g[0], want), (name, g[0], want)
        one = capi.median_f32(ws, v, l, drop_nan)
        assert one[0].tobytes() == g[0].tobytes() and one[1:] == g[1:], (name, one, g)
    return got


@pytest.mark.parametrize("drop_nan", [False, True])
def test_every_content_at_every_size(capi, ws, drop_nan):
    segs = segments()
    names = sorted(segs)
    rng = np.random.default_rng(93)
    names = [names[i] for i in rng.permutation(len(names))]            # sizes and contents mixed within a batch
    for at in range(0, len(names), 32):
        chunk = names[at:at + 32]
        run_and_check(capi, ws, chunk, segs, drop_nan, [i % 3 == 0 for i in range(len(chunk))])
    n_total = len(names)
    assert n_total == 16 * len(SIZES)


def test_only_nans_and_a_planted_nan(capi, ws):
    segs = segments()
    names = [f"only_nans_{n}" for n in SIZES] + [f"a_nan_{n}" for n in SIZES] + [f"normal_{n}" for n in SIZES]
    for drop_nan in (False, True):
        got = run_and_check(capi, ws, names, segs, drop_nan, [False] * len(names))
        for name, g in zip(names, got):
            n = int(name.rsplit("_", 1)[1])
            if name.startswith("only_nans"):
                assert np.isnan(g[0]) and g[2] == n and g[1] == (0 if drop_nan else n)
            elif name.startswith("a_nan"):
                assert g[2] == 1 and np.isnan(g[0]) == (not drop_nan or n == 1)
            else:
                assert g[2] == 0 and g[1] == n and np.isfinite(g[0])         # next to NaN rows, untouched


def test_with_and_without_locations_and_the_order_of_the_segments(capi, ws):
    segs = segments()
    names = ["normal_4099", "top_first_bin_257", "signed_zeros_2", "low_last_bin_256", "normal_1", "mid_spread_4099", "all_inf_3"]
    a = run_and_check(capi, ws, names, segs, False, [True, False, True, False, True, False, True])
    b = run_and_check(capi, ws, names[::-1], segs, False, [False] * len(names))
    none = run_and_check(capi, ws, names, segs, False, [False] * len(names))
    for x, y, z in zip(a, b[::-1], none):
        assert x[0].tobytes() == y[0].tobytes() == z[0].tobytes() and x[1:] == y[1:] == z[1:]
    assert run_and_check(capi, ws, ["normal_257"], segs, True, [True])[0][1] == 257          # B = 1
    assert capi.median_f32_batch(ws, []) == []
