"""sage_cycle_match_batch: one query descriptor map against B candidate maps.  Every output is an integer array, so row b is
demanded equal to the CPU oracle's cycle match of (query, candidate b, keypoints b), to sage_cycle_match on the same inputs,
to itself under every split of the target map into pixel slices, and to itself on a second call.

Shapes (C, H, W, K, B) -- the smallest at which each mechanism can fail:
  16, 32, 40,  37,  3   K not a multiple of the 8 queries of a workgroup
  32, 24, 24,   8,  1   H*W = 576: not a multiple of 256, nor of the 512 pixels a workgroup takes per step
  16, 64, 80, 200,  5   several steps per slice, 25 query groups, the largest case
  16, 16, 16,   8, 32   B = SAGE_MATCH_MAX_BATCH
Candidates, in turn: a shifted, noisy copy of the query map (as tests/test_gpu_parity.py::test_cycle_match_bit_exact builds
it); the query map itself; an unrelated map; a shifted copy again.  Every candidate has its own keypoint set.
Planted exact ties: in every candidate map the descriptor of the candidate's query 1 sits at the pixels 5 and H*W - 3 (any
split with two slices or more puts them into different slices; pixel 5 must win); the query map holds a duplicate pair
((7, 7) and (2, 9)), and query 0 of every candidate is the pixel (2, 9), whose twin sits in its own map.
pixel_slices: 0 (the library's choice), 1, 2, 7, 64 and H*W + 5 (clamped to one pixel per slice) at every shape; 7 divides
none of 1280, 576, 5120, 256."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32, 40, 37, 3), (32, 24, 24, 8, 1), (16, 64, 80, 200, 5), (16, 16, 16, 8, 32)]
THRESH = 2.0


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


@functools.lru_cache(maxsize=None)
def case(C_, H, W, K, B):
    rng = np.random.default_rng([11, C_, H, W, K, B])
    HW = H * W
    d0 = rng.standard_normal((C_, H, W)).astype(np.float32)
    d0[:, 7, 7] = d0[:, 2, 9]                                         # a duplicate pair inside the query map
    cands, kps = [], []
    for b in range(B):
        kp = rng.choice(HW, K, replace=False).astype(np.int64)       # the candidate's own keypoint set
        kp[0] = 2 * W + 9                                             # a query whose twin sits in its own map
        while kp[1] < 6 or kp[1] in (2 * W + 9, 7 * W + 7):           # (query 1 is the tie's: no copy of it in front of pixel 5)
            kp[1] += 6
        if b % 4 in (0, 3):
            d = np.roll(d0, (1 + b % 3, 2), axis=(1, 2)) + 0.05 * rng.standard_normal((C_, H, W)).astype(np.float32)
            if B == 1:                                                # (the only candidate: its upper half is unrelated, for flags of both kinds)
                d[:, :H // 2] = rng.standard_normal((C_, H // 2, W)).astype(np.float32)
        elif b % 4 == 1:
            d = d0.copy()
        else:
            d = rng.standard_normal((C_, H, W)).astype(np.float32)
        f = d.reshape(C_, HW)
        f[:, 5] = f[:, HW - 3] = d0.reshape(C_, HW)[:, kp[1]]         # an exact tie across any split: the first must win
        cands.append(np.ascontiguousarray(d)); kps.append(kp)
    for a in [d0] + cands + kps:
        a.setflags(write=False)
    return d0, cands, kps


@functools.lru_cache(maxsize=None)
def oracle_rows(C_, H, W, K, B):
    from oracle import oracle as orc
    orc.build()
    d0, cands, kps = case(C_, H, W, K, B)
    rows = [orc.cycle_match(d0, cands[b], kps[b], H, W, THRESH) for b in range(B)]
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def run(capi, ws, shape, slices):
    import torch
    C_, H, W, K, B = shape
    d0, cands, kps = case(*shape)
    cu = lambda a: torch.tensor(a).cuda()
    raw, cyc, fl, n, used = capi.cycle_match_batch(ws, cu(d0), [cu(c) for c in cands], [cu(k) for k in kps], H, W, THRESH, slices)
    return raw.cpu().numpy(), cyc.cpu().numpy(), fl.cpu().numpy(), n, used


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_equal_the_oracle(capi, orc, ws, shape):
    C_, H, W, K, B = shape
    om1, oc0, ofl = oracle_rows(*shape)
    raw, cyc, fl, n, used = run(capi, ws, shape, 0)
    assert used >= 1
    assert np.array_equal(raw, om1) and np.array_equal(cyc, oc0) and np.array_equal(fl, ofl)
    assert np.array_equal(n, ofl.sum(1)) and n.dtype == np.int32
    assert any(0 < int(ofl[b].sum()) < K for b in range(B)), "no candidate with flags of both kinds"
    assert (raw[:, 1] == 5).all()                                      # the tie at pixels 5 and H*W - 3: the first wins
    if B > 1:
        assert raw[1, 0] == 2 * W + 9                                  # the query map as candidate: (2, 9) before (7, 7)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_equal_the_single_call(capi, ws, shape):
    import torch
    C_, H, W, K, B = shape
    d0, cands, kps = case(*shape)
    raw, cyc, fl, n, _ = run(capi, ws, shape, 0)
    q = torch.tensor(d0).cuda()
    for b in range(B):
        m1, c0, f, cnt = capi.cycle_match(ws, q, torch.tensor(cands[b]).cuda(), torch.tensor(kps[b]).cuda(), H, W, THRESH)
        assert np.array_equal(raw[b], m1.cpu().numpy()) and np.array_equal(cyc[b], c0.cpu().numpy()), b
        assert np.array_equal(fl[b], f.cpu().numpy()) and n[b] == cnt, b


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_split_gives_the_same_arrays(capi, ws, shape):
    from tests.conftest import summary_line
    C_, H, W, K, B = shape
    om1, oc0, ofl = oracle_rows(*shape)
    used = {}
    for slices in (0, 1, 2, 7, 64, H * W + 5):
        raw, cyc, fl, n, used[slices] = run(capi, ws, shape, slices)
        assert np.array_equal(raw, om1) and np.array_equal(cyc, oc0) and np.array_equal(fl, ofl), slices
        assert np.array_equal(n, ofl.sum(1)), slices
    assert used[1] == 1 and used[2] == 2 and used[7] == 7 and used[H * W + 5] == H * W and used[64] == 64
    summary_line(f"cycle match batch {shape}: pixel_slices asked -> used " + ", ".join(f"{k} -> {v}" for k, v in used.items()))


def test_two_calls_give_identical_bytes_and_empty_calls_nothing(capi, ws):
    import torch
    shape = SHAPES[0]
    C_, H, W, K, B = shape
    a, b = run(capi, ws, shape, 0), run(capi, ws, shape, 3)
    c = run(capi, ws, shape, 0)
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    d0, cands, kps = case(*shape)
    cu = lambda t: torch.tensor(t).cuda()
    raw, cyc, fl, n, _ = capi.cycle_match_batch(ws, cu(d0), [], [], H, W, THRESH)
    assert raw.numel() == 0 and cyc.numel() == 0 and fl.numel() == 0 and n.size == 0
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    raw, cyc, fl, n, _ = capi.cycle_match_batch(ws, cu(d0), [cu(c_) for c_ in cands], [empty] * B, H, W, THRESH)
    assert raw.shape == (B, 0) and fl.shape == (B, 0) and np.array_equal(n, np.zeros(B, np.int32))
    again = run(capi, ws, shape, 0)                                    # (and the workspace is as good as before)
    assert again[0].tobytes() == a[0].tobytes() and np.array_equal(again[3], a[3])
