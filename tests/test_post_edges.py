"""The kernels of csrc/hhsr_post.hip (k_fc_median, k_fc_gauss, k_post_vblur, k_post_finish, k_orient_plane) and their
entry points at the borders of their arguments: one pixel, one row, one column, fewer rows or columns than blur taps,
windows wider than the image, tied and NaN samples, integer accumulated robustness (strengths that land on .5 and on exact
integers), every switch combination and every orientation with more than one workgroup.  References: the reference's own
outputs (golden "post_edges") and oracle/post.py, itself pinned on the CPU by tests/test_oracle_golden.py and
tests/test_post_ref.py.  Measured differences: PARITY.md, "Post path at its borders"."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import post_cases as pc
from helpers import assert_close
from oracle import post

pytestmark = pytest.mark.gpu

from handheld_super_resolution import _lib, raw2rgb, utils_image, config as hcfg  # noqa: E402

MFC = 8


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype).cuda()  # (a copy: the shared cases are read-only)


def N(t):
    return t.cpu().numpy()


def same_nan(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"


# ------------------------------------------------------------------------------------------------------ median denoiser
@pytest.mark.parametrize("tag", pc.GOLDEN_MEDIANS)
def test_median_golden(golden, tag):
    """The reference's own kernel on tied and NaN samples, integer robustness, radius up to 7, `mode: grey`, scale 1.5,
    one row / one column, radius 2.5 -> 2: bit for bit."""
    img, racc, cfg, scale, half, want = pc.golden_median_case(golden("post_edges"), tag)
    got = N(utils_image.frame_count_denoising_median(T(img), T(racc), hcfg.Config(cfg), scale=scale,
                                                     mode="grey" if half == 2 else "bayer"))
    same_nan(got, want, tag)
    assert_close(got, want, 0, 0, "median vs the reference's kernel, border cases")


# (index rule, scale) in every combination at radius_max 7 (the 225-sample window), three of them again at radius_max 5
# (r = 4 -> radius 2.5 -> 2), and a 3 x 4 robustness map that the indices leave (clamped)
MEDIAN_CASES = [(7, m, s, None) for m in pc.INDEX_MODES for s in (1, 1.5, 2)] + \
               [(5, "half", 1.5, None), (5, "nearest", 2, None), (5, "grey", 1, None),
                (7, "nearest", 1, (3, 4)), (5, "grey", 2, (3, 4))]


@pytest.mark.parametrize("radius_max,mode,scale,acc_shape", MEDIAN_CASES)
@pytest.mark.parametrize("shape", [(37, 53), (9, 131)])
def test_median_vs_oracle(shape, radius_max, mode, scale, acc_shape):
    H, W = shape
    half = pc.INDEX_MODES[mode]
    img = pc.quantised_image(H, W)
    racc = pc.integer_racc(*(acc_shape or pc.acc_reach(H, W, scale, half)), seed=radius_max)
    read = pc.acc_read(racc, H, W, scale, half)
    assert (read == 0).any() and (read == 4).any() and (read >= MFC).any()  # full radius, the .5 of radius_max 5, none
    if acc_shape:
        assert max(pc.acc_reach(H, W, scale, half)) > max(acc_shape)
    cfg = {"radius_max": radius_max, "max_frame_count": MFC}
    want = post.frame_count_denoising_median(img, racc, cfg, scale, half)
    got = N(utils_image.frame_count_denoising_median(T(img), T(racc), hcfg.Config(cfg), scale=scale,
                                                     half_index=bool(half), mode="grey" if half == 2 else "bayer"))
    same_nan(got, want, "median")
    assert_close(got, want, 0, 0, "median vs oracle: ties, NaN, integer robustness")


def test_median_radius_limit():
    """radius_max 7.4 rounds to 7 and runs; 7.5 rounds to 8 (half to even) and is refused like any radius above 7."""
    H, W = 9, 131
    img, racc = pc.quantised_image(H, W), pc.integer_racc(*pc.acc_reach(H, W, 2, True), seed=1)
    cfg = {"radius_max": 7.4, "max_frame_count": MFC}
    got = N(utils_image.frame_count_denoising_median(T(img), T(racc), hcfg.Config(cfg), scale=2))
    assert_close(got, post.frame_count_denoising_median(img, racc, cfg, 2), 0, 0, "median, radius_max 7.4")
    with pytest.raises(RuntimeError, match="overflows"):
        utils_image.frame_count_denoising_median(T(img), T(racc), hcfg.Config({"radius_max": 7.5, "max_frame_count": MFC}),
                                                 scale=2)


# ------------------------------------------------------------------------------------------------------- gauss denoiser
def _gauss(img, racc, sigma_max, scale, half, what):
    """Inputs in [0, 1]: the result is a weighted mean in [0, 1]; both sides round a float64 quotient that agrees to
    ~1e-13, so they differ by at most one float32 ulp below 1."""
    cfg = {"sigma_max": sigma_max, "max_frame_count": MFC}
    want = post.frame_count_denoising_gauss(img, racc, cfg, scale, half)
    got = N(utils_image.frame_count_denoising_gauss(T(img), T(racc), hcfg.Config(cfg), scale=scale, half_index=bool(half),
                                                    mode="grey" if half == 2 else "bayer"))
    same_nan(got, want, what)
    assert_close(got, want, 0, pc.ULP1, what)
    return want


@pytest.mark.parametrize("sigma_max", [1.5, 4])
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_gauss_vs_oracle(shape, sigma_max):
    """Every shape; with sigma_max 4 the window reaches 25 x 25 — wider than (5, 70) and (2, 9) — and r = 6 gives
    sigma = 1, 3 sigma = 3.0 exactly (ceil must not add a tap); r >= 8 gives sigma = 0 (the pixel itself)."""
    H, W = shape
    img = pc.unit_image(H, W)
    racc = pc.integer_racc(*pc.acc_reach(H, W, 2, True))
    read = pc.acc_read(racc, H, W, 2, True)
    sigma = sigma_max * (MFC - np.minimum(read, MFC)) / MFC
    if sigma_max == 4:
        assert (sigma == 1.0).any()
    if H * W > 1:  # (one pixel reads one robustness value, the 6 of integer_racc: it cannot also read one >= 8)
        assert (sigma == 0.0).any()
    want = _gauss(img, racc, sigma_max, 2, True, "gauss vs oracle, every shape")
    assert np.array_equal(want[sigma == 0], img[sigma == 0])


@pytest.mark.parametrize("mode,scale", [("nearest", 1.5), ("grey", 2), ("grey", 1.5), ("half", 1)])
def test_gauss_index_rules_and_nan(mode, scale):
    """The other index rules and scales, a 3 x 4 robustness map (clamped indices) and two NaN pixels: each spreads over
    the windows that contain it and no further."""
    H, W = 37, 53
    half = pc.INDEX_MODES[mode]
    img = pc.unit_image(H, W, seed=1, nans=2)
    ys, xs = np.mgrid[:H, :W]
    for racc in (pc.integer_racc(*pc.acc_reach(H, W, scale, half), seed=2), pc.integer_racc(3, 4, seed=2)):
        want = _gauss(img, racc, 4, scale, half, "gauss vs oracle, index rules, two NaN pixels")
        # a pixel is NaN exactly where its own window, t = ceil(3 sigma) to each side, holds a NaN pixel
        t = np.ceil(3 * 4 * (MFC - np.minimum(pc.acc_read(racc, H, W, scale, half), MFC)) / MFC)
        reached = np.zeros((H, W), bool)
        for ny, nx in zip(*np.nonzero(np.isnan(img[..., 0]))):
            reached |= np.maximum(abs(ys - ny), abs(xs - nx)) <= t
        assert reached.sum() > 2 and np.array_equal(np.isnan(want), np.repeat(reached[..., None], 3, -1))


# ------------------------------------------------------------------------------------------------------------ postprocess
SHARPEN = {"r3": {"enabled": True, "radius": 3, "amount": 1.5},     # 12 taps: more than the rows of four of the shapes
           "r05": {"enabled": True, "radius": 0.5, "amount": 0.5},  # 2 taps
           "r16": {"enabled": True, "radius": 16, "amount": 0.5}}   # 64 taps, the ABI limit: > 6 reflection periods of 5 rows
OFF = {"enabled": False}


def _postprocess(img, ccm, sharpen, devig, what):
    """One switch combination in two steps (the gamma curve has unbounded slope at 0: a 3e-7 colour-matrix difference at
    a clipped pixel would become 1e-3): the linear result against the oracle at the project's bounds, then the gamma
    result against float32 x^(1/2.2) of the GPU's own linear result."""
    sh = SHARPEN.get(sharpen, OFF)
    atol, kind = (1e-6, "no sharpening") if sharpen is None else (4e-6, "sharpening, then devignetting") if devig else \
        (2e-6, "sharpening")
    lin = N(raw2rgb.postprocess(None, T(img), ccm, False, False, hcfg.Config(sh), devig, pc.XYZ2CAM))
    want = post.postprocess(img, ccm, False, False, sh, devig, pc.XYZ2CAM)
    same_nan(lin, want, what)
    assert_close(lin, want, 0, atol, f"postprocess, linear result, {kind}")
    gam = N(raw2rgb.postprocess(None, T(img), ccm, False, True, hcfg.Config(sh), devig, pc.XYZ2CAM))
    same_nan(gam, lin, what)
    assert_close(gam, np.clip(lin ** pc.F32(1.0 / 2.2), 0, 1), 0, 1e-6, "postprocess, gamma of the GPU's linear result")
    if not ccm and sharpen is None and not devig:
        want = post.postprocess(img, False, False, True, OFF, False, pc.XYZ2CAM)
        same_nan(gam, want, what)
        assert_close(gam, want, 0, 1e-6, "postprocess, gamma only, vs oracle")
    return lin


@pytest.mark.parametrize("ccm,sharpen,devig", list(itertools.product([False, True], [None, "r3"], [False, True])))
@pytest.mark.parametrize("shape", [(37, 53), (2, 9)])
def test_postprocess_switch_matrix(shape, ccm, sharpen, devig):
    """All 16 combinations of (colour matrix, sharpening, devignetting, gamma); the input has exact 0.0 and 1.0 blocks,
    values outside [0, 1] and a NaN pixel."""
    lin = _postprocess(pc.post_image(*shape), ccm, sharpen, devig, "switch matrix")
    assert np.isnan(lin).any()
    if sharpen:  # (the NaN pixel takes its whole 25 x 25 window with it: the small shape again without it)
        lin = _postprocess(pc.post_image(*shape, nan=False), ccm, sharpen, devig, "switch matrix, no NaN")
        assert not np.isnan(lin).any()


@pytest.mark.parametrize("sharpen", list(SHARPEN))
@pytest.mark.parametrize("shape", pc.SHAPES)
def test_postprocess_full_every_shape(shape, sharpen):
    """Colour matrix + sharpening + devignetting + gamma at every shape (H == 1 and W == 1 branches of the gain, fewer
    rows / columns than taps: reflect() beyond its first period) for 2, 12 and 64 taps; with the NaN pixel and without
    (with it the blur leaves little of the small images finite)."""
    _postprocess(pc.post_image(*shape), True, sharpen, True, "full")
    lin = _postprocess(pc.post_image(*shape, nan=False), True, sharpen, True, "full, no NaN")
    assert not np.isnan(lin).any()


def test_postprocess_tap_limit():
    """radius 16.2 means 65 taps: one more than the ABI carries."""
    img = T(pc.post_image(5, 70))
    with pytest.raises(RuntimeError, match="invalid argument"):
        raw2rgb.postprocess(None, img, True, False, True, hcfg.Config({"enabled": True, "radius": 16.2, "amount": 0.5}), True,
                            pc.XYZ2CAM)


# ------------------------------------------------------------------------------------------------------------ orientation
@pytest.mark.parametrize("ori", range(1, 9))
@pytest.mark.parametrize("shape", [(5, 70), (9, 131), (1, 7)])
def test_orientation(shape, ori):
    """k_orient_plane ([H, W] planes), the tensor route ([H, W, 3]) and the store of k_post_finish against the oracle's
    apply_orientation: index maps only, so bit for bit — the post-process store against the orientation of the GPU's own
    un-oriented result."""
    H, W = shape
    img = pc.post_image(H, W, seed=3, nan=False)
    want = np.ascontiguousarray(post.apply_orientation(img, ori))
    assert_close(N(utils_image.apply_orientation(T(img[..., 0]), ori)), want[..., 0], 0, 0, "orientation of a plane")
    assert_close(N(utils_image.apply_orientation(T(img), ori)), want, 0, 0, "orientation of an image")
    sharp = hcfg.Config(SHARPEN["r3"])
    base = N(raw2rgb.postprocess(None, T(img), True, False, True, sharp, True, pc.XYZ2CAM, orientation=1))
    got = N(raw2rgb.postprocess(None, T(img), True, False, True, sharp, True, pc.XYZ2CAM, orientation=ori))
    assert_close(got, np.ascontiguousarray(post.apply_orientation(base, ori)), 0, 0, "orientation in the post-process store")


# ----------------------------------------------------------------------------------------------------- argument refusals
SENTINEL = -7.25


class _Buffers:
    def __init__(self, H=5, W=9):
        self.H, self.W = H, W
        self.img = T(pc.unit_image(H, W))
        self.acc = T(np.asarray(pc.integer_racc(3, 5)))
        self.taps, self.radius = raw2rgb._device_taps(0.5, self.img.device)
        self.out = torch.full((H, W, 3), SENTINEL, device="cuda")
        self.tmp = torch.full((H, W, 3), SENTINEL, device="cuda")
        self.keep = self.img.clone()

    def refused(self, name, *args):
        with pytest.raises(RuntimeError, match=f"{name} failed"):
            _lib.call(name, *args)
        torch.cuda.synchronize()
        assert bool((self.out == SENTINEL).all()) and bool((self.tmp == SENTINEL).all()), f"{name}: output written"
        assert torch.equal(self.img, self.keep), f"{name}: input written"


def test_frame_count_denoise_refusals():
    b = _Buffers()
    p, st, NULL = _lib.ptr, _lib.stream(), ctypes.c_void_p(0)

    def args(image=None, out=None, acc=None, scale=2.0, kind=0, strength=3.0, mfc=8.0):
        return (p(b.img) if image is None else image, p(b.out) if out is None else out, b.H, b.W,
                p(b.acc) if acc is None else acc, 3, 5, scale, kind, strength, mfc, 1, st)

    for kw in (dict(image=NULL), dict(out=NULL), dict(acc=NULL), dict(out=p(b.img)), dict(scale=0.99), dict(mfc=0.0),
               dict(mfc=-1.0), dict(strength=-0.5), dict(kind=2), dict(kind=-1)):
        b.refused("hhsr_frame_count_denoise", *args(**kw))
    for kind in (0, 1):  # and the same call with nothing wrong runs
        _lib.call("hhsr_frame_count_denoise", *args(kind=kind))
    torch.cuda.synchronize()
    assert not bool((b.out == SENTINEL).any())


def test_postprocess_refusals():
    b = _Buffers()
    p, st, NULL = _lib.ptr, _lib.stream(), ctypes.c_void_p(0)

    def args(tmp=None, out=None, sharpen=1, taps=None, radius=None, ori=1):
        return (p(b.img), p(b.tmp) if tmp is None else tmp, p(b.out) if out is None else out, b.H, b.W, None, sharpen, 0.5,
                p(b.taps) if taps is None else taps, b.radius if radius is None else radius, 0, 1, ori, st)

    for kw in (dict(ori=0), dict(ori=9), dict(out=p(b.img)), dict(ori=0, sharpen=0), dict(ori=9, sharpen=0),
               dict(out=p(b.img), sharpen=0), dict(tmp=NULL), dict(taps=NULL), dict(radius=65), dict(radius=-1),
               dict(tmp=p(b.img)), dict(tmp=p(b.out))):
        b.refused("hhsr_postprocess", *args(**kw))
    _lib.call("hhsr_postprocess", *args(sharpen=0, tmp=NULL, taps=NULL))  # without sharpening neither is needed
    _lib.call("hhsr_postprocess", *args())
    torch.cuda.synchronize()
    assert not bool((b.out == SENTINEL).any()) and not bool((b.tmp == SENTINEL).any())


def test_orient_plane_refusals():
    b = _Buffers()
    p, st = _lib.ptr, _lib.stream()
    plane, out = b.img[..., 0].contiguous(), b.out[..., 0].contiguous()
    keep = plane.clone()
    for src, dst, ori in ((plane, plane, 6), (plane, out, 9), (plane, out, 0)):
        with pytest.raises(RuntimeError, match="hhsr_orient_plane failed"):
            _lib.call("hhsr_orient_plane", p(src), p(dst), b.H, b.W, ori, st)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and torch.equal(plane, keep)
    _lib.call("hhsr_orient_plane", p(plane), p(out), b.H, b.W, 6, st)
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
