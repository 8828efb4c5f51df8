"""The keyframe ingest producers (producers.hip and their entry points in operators.hip) at their edge shapes:
sage_depth_and_grad, sage_gaussian_pyramid_with_grad, sage_valid_locations, sage_sample_locations, sage_sort_locations.

depth_and_grad, CS = 16 and 32 (depth_kernel<16> has no other test), on 50x62 (3100 pixels: no multiple of the 32 / 64
pixels a workgroup covers), 3x5 and 64x80.  Depth against orc.update_depth(prec="f64"): max abs error <= 4 x the fp32
oracle's own max abs error on the case.  Gradient: bit-equal to synth.spatial_grad of the kernel's own depth --
0.5f * (a - b) is one correctly rounded subtraction and an exact halving, every IEEE implementation agrees -- which
checks every border texel exactly.  grad = NULL is accepted.

gaussian_pyramid_with_grad on 40x56 L = 4 FS = 16 (last level 5x7), 32x40 L = 3 FS = 32, 64x80 L = 1 and L = 2, 50x62
L = 2 (last level 25x31), under four masks: all ones, the synthetic video mask, a holey one (20 % random holes and a dead
rectangle: texels without a live tap and with some, tests/test_edge_scenes.py) and all zeros.  Level 0 is bit-equal to
the input; every level's gradient is bit-equal to synth.spatial_grad of the kernel's own level; every level l + 1 is
checked one step at a time -- the kernel's own level l and the numpy-decimated mask m[::2, ::2] go to the fp64 oracle as
a two-level pyramid, max abs error <= 4 x the fp32 oracle's for the same step -- so that rounding does not compound down
the pyramid and a wrong decimated mask shows at the level after it; texels whose nine mask taps are zero are exactly 0;
everything is finite.  An odd intermediate level (50x62, L = 3) is SAGE_E_UNSUPPORTED and writes nothing.

valid_locations on 24x32 (below one 1024-pixel chunk), 32x32 (one chunk), 25x41 (one chunk + 1) and 50x62 under six masks
(zeros, ones, random, only the last pixel, only the last partial chunk, values around the 0.5 threshold): locations and
coordinates bit-equal to the oracle.  sample_locations at n_valid = 1 and num_samples = 0.  sort_locations on 50x62 at
n = 0, 1, 500, 3100 against argsort, a duplicate pair across two chunks (order kept, ok = False), a location = H W (raises).

Measured on an MI355X: the kernel's max abs error as a share of its bar (4 x the fp32 oracle's own), worst over the
cases of a row

  depth   50x62  CS16 0.250 (1.40e-07 of 5.60e-07)   CS32 0.215 (1.50e-07 of 6.97e-07)
  depth   3x5    CS16 0.250 (1.10e-07 of 4.38e-07)   CS32 0.164 (9.60e-08 of 5.84e-07)
  depth   64x80  CS16 0.250 (1.52e-07 of 6.09e-07)   CS32 0.237 (1.63e-07 of 6.89e-07)
  pyramid every shape with a second level, masks ones / synthetic / holey: 0.250; mask zeros: 0 of 0
  (0.250: the kernel's worst texel is as far from fp64 as the fp32 oracle's)

With W in place of W - 1 in the gradient clamps every depth and every pyramid case fails on the gradient's bit-equality.
"""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import edge_scenes as es
from tests.conftest import summary_line

pytestmark = pytest.mark.gpu

SAGE_E_UNSUPPORTED = -2


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


def _dv(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("CS", [16, 32])
@pytest.mark.parametrize("H,W", es.DEPTH_SHAPES, ids=lambda v: str(v))
def test_depth_and_grad_shapes(capi, ws, orc, H, W, CS):
    import torch
    bias, basis, code, scale = es.depth_inputs(H, W, CS)
    d64 = orc.update_depth(bias, basis, code, scale, prec="f64").reshape(H, W)
    d32 = orc.update_depth(bias, basis, code, scale).reshape(H, W)
    bar = 4 * _maxabs(d32, d64)
    bd, sd = _dv(bias), _dv(basis)
    dpt, grad = capi.depth_and_grad(ws, bd, sd, code, scale, H, W, CS)
    dpt, grad = dpt.cpu().numpy(), grad.cpu().numpy()
    got = _maxabs(dpt, d64)
    summary_line(f"producer shapes depth {H}x{W} CS{CS}: max abs error {got:.3e}, bar {bar:.3e}, share {got / bar:.3f}")
    assert got <= bar
    assert np.array_equal(grad, synth.spatial_grad(dpt[None])[:, 0])
    # grad = NULL: the depth alone, the same bits
    only = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
    code_d = _dv(code)
    rc = capi.lib().sage_depth_and_grad(ws.h, capi.dptr(only), C.c_void_p(0), capi.dptr(bd), capi.dptr(sd), capi.dptr(code_d),
                                        C.c_float(scale), H, W, CS)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(only.cpu().numpy(), dpt)


# --------------------------------------------------------------------------------------------------------------------
def _pyr_id(c):
    return f"{c['H']}x{c['W']}_L{c['L']}_FS{c['FS']}"


@pytest.mark.parametrize("kind", es.MASK_KINDS)
@pytest.mark.parametrize("case", es.PYRAMID_CASES, ids=_pyr_id)
def test_gaussian_pyramid_shapes(capi, ws, orc, case, kind):
    H, W, L, FS = case["H"], case["W"], case["L"], case["FS"]
    feat, mask = es.pyramid_feat(H, W, FS), es.pyramid_mask(kind, H, W)
    cams = synth.camera_pyramid(synth.Camera(0.9 * W, 0.9 * W, W / 2.0, H / 2.0, W, H), L)
    offs, P = synth.level_offsets_of(cams)
    pyr = capi.make_pyramid(cams[0], L)
    assert pyr.P == P and [pyr.level_offsets[l] for l in range(L)] == list(offs)
    hp, hg = capi.gaussian_pyramid_with_grad(ws, _dv(feat), _dv(mask), pyr, FS)
    hp, hg = hp.cpu().numpy(), hg.cpu().numpy()
    assert np.isfinite(hp).all() and np.isfinite(hg).all()
    sizes = [(int(c.h), int(c.w)) for c in cams]
    levels = [hp[:, offs[l]:offs[l] + h * w].reshape(FS, h, w) for l, (h, w) in enumerate(sizes)]
    assert np.array_equal(levels[0], feat)
    masks = es.mask_levels(mask, L)
    worst = 0.0
    for l, (h, w) in enumerate(sizes):
        g = hg[:, :, offs[l]:offs[l] + h * w].reshape(2, FS, h, w)
        assert np.array_equal(g, synth.spatial_grad(levels[l])), f"gradient of level {l}"
        if l + 1 == L:
            break
        assert masks[l].shape == (h, w)
        n2 = sizes[l + 1][0] * sizes[l + 1][1]
        two = np.array([0, h * w], np.int32)
        o64, _ = orc.gaussian_pyramid_with_grad(levels[l], masks[l], 2, two, h * w + n2, prec="f64")
        o32, _ = orc.gaussian_pyramid_with_grad(levels[l], masks[l], 2, two, h * w + n2)
        want, own = o64[:, h * w:].reshape(levels[l + 1].shape), o32[:, h * w:].reshape(levels[l + 1].shape)
        bar, got = 4 * _maxabs(own, want), _maxabs(levels[l + 1], want)
        worst = max(worst, got / bar if bar > 0 else (0.0 if got == 0 else np.inf))
        assert got <= bar, f"level {l + 1}: max abs error {got:.3e} against a bar of {bar:.3e}"
        live, _ = es.live_taps(masks[l])
        dead = live == 0
        assert not levels[l + 1][:, dead].any(), f"level {l + 1}: a texel without a live mask tap is not 0"
    summary_line(f"producer shapes pyramid {_pyr_id(case)} {kind}: worst share of the bar {worst:.3f}")


def test_gaussian_pyramid_odd_intermediate_level_is_unsupported(capi, ws):
    import torch
    H, W, L, FS = 50, 62, 3, 16
    pyr = capi.make_pyramid(synth.Camera(0.9 * W, 0.9 * W, W / 2.0, H / 2.0, W, H), L)
    out = torch.full((FS, pyr.P), 7.0, dtype=torch.float32, device="cuda")
    grad = torch.full((2, FS, pyr.P), 7.0, dtype=torch.float32, device="cuda")
    rc = capi.lib().sage_gaussian_pyramid_with_grad(ws.h, capi.dptr(out), capi.dptr(grad), capi.dptr(_dv(es.pyramid_feat(H, W, FS))),
                                                    capi.dptr(_dv(es.pyramid_mask("ones", H, W))), C.byref(pyr), FS)
    torch.cuda.synchronize()
    assert rc == SAGE_E_UNSUPPORTED
    assert bool((out == 7.0).all()) and bool((grad == 7.0).all())


# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", es.LOCATION_SHAPES, ids=lambda v: str(v))
def test_valid_locations_chunks(capi, ws, orc, H, W):
    cam = es.location_camera(H, W)
    scam = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    for kind in es.LOCATION_MASKS:
        m = es.location_mask(kind, H, W)
        oloc, ohomo = orc.valid_locations(m, cam)
        hloc, hhomo = capi.valid_locations(ws, _dv(m), scam)
        assert np.array_equal(hloc.cpu().numpy(), oloc), kind
        assert np.array_equal(hhomo.cpu().numpy(), ohomo), kind
        if (H, W) != (50, 62) or len(oloc) == 0:
            continue
        # the seeded subsample behind it: one valid pixel, and no sample asked for
        if kind == "last_pixel":
            sloc, shomo = capi.sample_locations(ws, hloc, hhomo, 11, 300)
            assert np.array_equal(sloc.cpu().numpy(), oloc) and np.array_equal(shomo.cpu().numpy(), ohomo) and len(oloc) == 1
        sloc, shomo = capi.sample_locations(ws, hloc, hhomo, 11, 0)
        assert sloc.shape[0] == 0 and shomo.shape[0] == 0


def test_sort_locations_chunks(capi, ws):
    H, W = 50, 62
    HW = H * W
    rng = np.random.default_rng(4)
    for n in (0, 1, 500, HW):
        loc = rng.permutation(HW)[:n].astype(np.int64)
        homo = rng.normal(size=(n, 3)).astype(np.float32)
        lo, ho, ok = capi.sort_locations(ws, _dv(loc), _dv(homo), H, W)
        order = np.argsort(loc)
        assert ok, n
        assert np.array_equal(lo.cpu().numpy(), loc[order]) and np.array_equal(ho.cpu().numpy(), homo[order]), n
    # a pixel listed twice, by entries 5 and 2 * 1024 + 20 of the list (two chunks apart); every other pixel but one is
    # listed once, the duplicated pixel lies in the last, partial chunk of the image: the caller's order is kept
    loc2 = loc.copy()
    loc2[5] = loc2[2 * es.CHUNK + 20] = 3 * es.CHUNK + 20
    assert len(np.unique(loc2)) < HW
    lo, ho, ok = capi.sort_locations(ws, _dv(loc2), _dv(homo), H, W)
    assert not ok and np.array_equal(lo.cpu().numpy(), loc2) and np.array_equal(ho.cpu().numpy(), homo)
    loc3 = loc.copy()
    loc3[HW - 1] = HW                                     # the first location outside the image
    with pytest.raises(capi.SageError):
        capi.sort_locations(ws, _dv(loc3), _dv(homo), H, W)
