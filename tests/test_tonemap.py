"""Tone mapping on the GPU (hhsr_post_expose, hhsr_mertens, raw2rgb.postprocess(do_tonemapping=True), process())
against the NumPy restatement of the contract, tests/mertens_ref.py.

Bounds: exposures and normalised weights are decision stages and compared at tolerance 0.  The fused image is compared
with the restatement blended in float64 on the same float32 weights; the bound is 4 x the spread between the
restatement's own float32 and float64 blends of the same inputs (computed here, ~2e-7 - 4e-7, so ~1e-6): the factor
allows for the kernels' different summation order.  Measured values: PARITY.md."""
import ctypes

import numpy as np
import pytest
import torch

import mertens_ref as ref
from helpers import assert_close
from tonemap_cases import F32, SHAPES, case, image, log_figure

pytestmark = pytest.mark.gpu

from handheld_super_resolution import _lib, raw2rgb, config as hcfg  # noqa: E402

XYZ2CAM = np.array([[0.9, -0.3, -0.1], [-0.4, 1.2, 0.2], [-0.1, 0.2, 0.6]])


def T(a):
    return torch.as_tensor(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def N(t):
    return t.cpu().numpy()


def expose(img, ccm=None, sharpen=None, devignette=False, times=ref.TIMES):
    """hhsr_post_expose on a float32 [H][W][3] array: uint8 [n][H][W][3]."""
    img = T(np.asarray(img, F32))
    H, W, _ = img.shape
    n = len(times)
    taps, tr, tmp, amount = None, 0, None, 0.0
    if sharpen is not None:
        taps, tr = raw2rgb._device_taps(sharpen["radius"], img.device)
        tmp, amount = torch.empty_like(img), sharpen["amount"]
    out = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=img.device)
    _lib.call("hhsr_post_expose", _lib.ptr(img), _lib.ptr(tmp), H, W, None if ccm is None else _lib.floats(np.ravel(ccm)),
              int(sharpen is not None), float(amount), _lib.ptr(taps), int(tr), int(devignette), _lib.doubles(times), n,
              _lib.ptr(out), _lib.stream(img.device))
    return N(out)


def mertens(expo, smoothstep, want_weights=True):
    """hhsr_mertens on uint8 [n][H][W][3]: (fused float32 [H][W][3], normalised weights [n][H][W] or None).  The
    workspace is allocated with a guard band behind it, which must come back untouched."""
    n, H, W, _ = expo.shape
    nbytes, levels = ctypes.c_size_t(), ctypes.c_int()
    _lib.call("hhsr_tonemap_workspace", H, W, n, nbytes, levels)
    assert levels.value == ref.levels(H, W)
    e = T(expo)
    work = torch.full((nbytes.value + 256,), 0xA5, dtype=torch.uint8, device=e.device)
    out = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device=e.device)
    wts = torch.full((n, H, W), float("nan"), dtype=torch.float32, device=e.device) if want_weights else None
    _lib.call("hhsr_mertens", _lib.ptr(e), n, H, W, _lib.ptr(work), nbytes.value, _lib.ptr(wts), _lib.ptr(out),
              int(smoothstep), _lib.stream(e.device))
    assert (N(work[nbytes.value:]) == 0xA5).all(), "write behind the workspace"
    return N(out), (N(wts) if want_weights else None)


def wide_image(H, W, seed=0):
    """`image` stretched to [-0.2, 1.6], values below 0 and above 1 in the first and last pixel whatever the shape."""
    img = image(H, W, seed, -0.2, 1.6)
    img[0, 0] = (-0.2, 1.6, 0.5)
    img[-1, -1] = (1.5, -0.1, 1.2)
    return img


@pytest.mark.parametrize("shape", SHAPES)
def test_exposures_float32(shape):
    """Comparison 1: no colour matrix, sharpening or devignetting — the float32 path, tolerance 0."""
    img = wide_image(*shape)
    assert (img < 0).any() and (img > 1).any()
    got = expose(img)
    assert got.dtype == np.uint8 and np.array_equal(got, ref.exposures(img))


@pytest.mark.parametrize("shape", SHAPES)
def test_exposures_after_devignetting_are_float64_and_unclipped(shape):
    """Comparison 2: with devignetting the image is float64 upstream (float64 gain x float32 image) and reaches the
    0.5 x exposure unclipped; tolerance 0.  The gain's cos() may differ from NumPy's in its last bit (1e-16 relative);
    the inputs are checked to sit 1e-9 away from every rounding tie, so that cannot move a value."""
    from oracle import post

    img = wide_image(*shape, seed=3)
    d = post.devignette(img)
    assert d.dtype == np.float64 and (d > 1).any()
    for t in ref.TIMES:
        v = np.clip(d * t, 0, 1) * 255
        assert np.abs(v - np.floor(v) - 0.5).min() > 1e-9
    want = ref.exposures(d)
    assert not np.array_equal(want, ref.exposures(np.clip(d, 0, 1)))          # clipping first is another result
    assert np.array_equal(expose(img, devignette=True), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_normalised_weights(shape):
    """Comparison 3: the weight maps are a decision stage — bit for bit."""
    c = case(shape)
    _, wn = mertens(c["expo"], smoothstep=False)
    assert_close(wn, c["wn"], 0, 0, "mertens: normalised weights")


@pytest.mark.parametrize("smoothstep", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_image(shape, smoothstep):
    """Comparison 4: against the restatement blended in float64 on the same float32 weights; bound = 4 x the spread of
    the restatement's float32 blend around it."""
    c = case(shape)
    spread = c["spread_smooth" if smoothstep else "spread"]
    assert spread > 0
    got, _ = mertens(c["expo"], smoothstep, want_weights=False)
    log_figure(f"mertens: float32 vs float64 spread of the restatement, smoothstep {smoothstep}", spread, 4 * spread, got.size)
    assert_close(got, c["s64" if smoothstep else "r64"], 0, 4 * spread, f"mertens: fused image, smoothstep {smoothstep}")


@pytest.mark.parametrize("n", [1, 3, 4])
@pytest.mark.parametrize("shape", [(37, 53), (16, 16), (131, 259)])
def test_identical_exposures_fuse_to_the_exposure(shape, n):
    """Comparison 5: partition of unity, within the bound of comparison 4 for the same shape."""
    c = case(shape)
    e = np.stack([c["expo"][2]] * n)
    got, _ = mertens(e, smoothstep=False, want_weights=False)
    assert_close(got, ref.to_float(e[0]), 0, 4 * c["spread"], "mertens: n identical exposures")


# 33540 pixels: the 1e-3 cap on exposure near-ties is 33 pixels.  Even sizes: with an odd one the devignetting gain is
# exactly 1 on the centre row / column, where every saturated pixel (exactly 1.0 after the colour matrix's clip) is an
# exact tie of the 0.5 x exposure (127.5): exact on both sides, but the one-ulp check below counts them.
POST_SHAPE = (130, 258)
SHARP = {"enabled": True, "radius": 2, "amount": 1.5}
POST_CASES = {  # name: (colour matrix, sharpening, devignetting, gamma, orientation)
    "plain": (False, None, False, False, 1),
    "ccm_sharp_ori6": (True, SHARP, False, False, 6),
    "ccm_devig_gamma": (True, None, True, True, 1),
    "sharp_devig_gamma_ori6": (False, SHARP, True, True, 6),
}


def upstream_chain(img, ccm, sharpen):
    """The reference's float32 steps before the devignetting (raw2rgb.py:221-238), composed from the oracle's."""
    from oracle import post

    if ccm:
        img = np.clip(post.apply_ccm(img, np.linalg.inv(post.get_color_matrix(XYZ2CAM))), 0.0, 1.0)
    if sharpen:
        img = post.unsharp_mask(img, sharpen["radius"], sharpen["amount"])
    assert img.dtype == F32
    return img


def chain_exposures(pre, devignette):
    from oracle import post

    return ref.exposures(post.devignette(pre) if devignette else pre)


def near_tie_pixels(pre, devignette):
    """Pixels where some exposure changes when the float32 image before the devignetting moves by one ulp, up or down."""
    e = chain_exposures(pre, devignette)
    lo = chain_exposures(np.nextafter(pre, F32(-np.inf)), devignette)
    hi = chain_exposures(np.nextafter(pre, F32(np.inf)), devignette)
    return ((e != lo) | (e != hi)).any(axis=(0, 3))


@pytest.mark.parametrize("name", list(POST_CASES))
def test_postprocess_with_tone_mapping(name):
    """Comparison 6: raw2rgb.postprocess(do_tonemapping=True, restated_tonemapping=True) against the chain composed from the oracle's colour matrix,
    unsharp mask and devignetting and the restatement.  Upstream float32 rounding can flip a rint near-tie, so the
    GPU's exposures may differ from the chain's by 1 LSB on at most 1e-3 of the pixels (the inputs are checked: one ulp
    at the restatement's input moves far fewer); the fused image is then compared as in comparison 4 against the
    restatement run on the GPU's own exposures, and the gamma curve against the GPU's own result without it."""
    from oracle import post

    ccm, sharpen, devignette, gamma, ori = POST_CASES[name]
    H, W = POST_SHAPE
    img = wide_image(H, W, seed=7) if not ccm else image(H, W, 7, 0.0, 1.2)
    pre = upstream_chain(img, ccm, sharpen)
    cap = int(1e-3 * H * W)
    assert near_tie_pixels(pre, devignette).sum() < cap
    want_e = chain_exposures(pre, devignette)
    cam2rgb = np.linalg.inv(raw2rgb.get_color_matrix(None, XYZ2CAM)).astype(F32) if ccm else None
    got_e = expose(img, cam2rgb, sharpen, devignette)
    de = np.abs(got_e.astype(np.int16) - want_e.astype(np.int16))
    log_figure(f"postprocess + tone mapping: pixels with an exposure 1 LSB off, {name}", int((de > 0).any(axis=(0, 3)).sum()), cap, H * W)
    assert de.max() <= 1 and (de > 0).any(axis=(0, 3)).sum() <= cap
    if not (ccm or sharpen):
        assert de.max() == 0

    cfg = hcfg.Config(sharpen) if sharpen else None
    got = N(raw2rgb.postprocess(None, T(img), ccm, True, False, cfg, devignette, XYZ2CAM, orientation=ori, restated_tonemapping=True))
    f32, _ = ref.mertens(got_e, smooth=True, dtype=F32)
    f64, _ = ref.mertens(got_e, smooth=True, dtype=np.float64)
    spread = float(np.abs(f32 - f64).max())
    want = post.apply_orientation(np.clip(f64, 0.0, 1.0), ori)
    assert got.shape == want.shape and got.dtype == np.float32
    assert_close(got, want, 0, 4 * spread, f"postprocess + tone mapping, {name}")
    if gamma:
        got_g = N(raw2rgb.postprocess(None, T(img), ccm, True, True, cfg, devignette, XYZ2CAM, orientation=ori, restated_tonemapping=True))
        # float32 powf of the clipped fused image (raw2rgb.py:245-249): 1e-6 as for the gamma of the existing post path
        assert_close(got_g, np.clip(got ** F32(1.0 / 2.2), 0, 1), 0, 1e-6, f"postprocess + tone mapping + gamma, {name}")
    with pytest.raises(NotImplementedError):  # the plain switch means OpenCV, which this build does not have
        raw2rgb.postprocess(None, T(img), ccm, True, False, cfg, devignette, XYZ2CAM, orientation=ori)
    with pytest.raises(AssertionError):
        raw2rgb.postprocess(None, T(img[..., :2]), False, True, False, None, restated_tonemapping=True)  # non-3-channel: refused


def test_process_with_tone_mapping():
    """Comparison 7: process() with postprocessing.do_tonemapping returns and is bit-identical to postprocess(main());
    with the switch off (the default) it is bit-identical to the post path without tone mapping."""
    import handheld_super_resolution as hsr
    from handheld_super_resolution import synthetic as synth

    assert hsr.default_config().postprocessing.do_tonemapping is False
    ref_raw, comp, _ = synth.make_burst(128, 160, 3, seed=11, max_shift=1.5)
    std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    burst = {"ref": ref_raw, "comp": comp, "cfa_pattern": [[0, 1], [1, 2]], "white_balance": [1.0, 1.0, 1.0],
             "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "std_curve": std, "diff_curve": diff, "orientation": 6}
    outs = {}
    for on in (True, False):
        cfg = hsr.default_config()
        cfg.verbose = 0
        cfg.block_matching.tuning.tile_size = 16
        cfg.block_matching.tuning.factors = [1, 2, 2, 2]
        cfg.block_matching.tuning.metrics = ["L2"] * 4
        cfg.postprocessing.do_tonemapping = on
        cfg.postprocessing.do_color_correction = False
        img, _ = hsr.process(burst, cfg)
        merged, _ = hsr.main(ref_raw, comp, cfg)
        pp = cfg.postprocessing
        want = raw2rgb.postprocess(None, merged, False, on, pp.do_gamma_correction, pp.sharpening, pp.do_devignetting,
                                   orientation=6, restated_tonemapping=True)
        assert img.shape == tuple(want.shape) and img.shape[0] > img.shape[1]  # orientation 6: [W][H][3]
        assert np.array_equal(img, N(want), equal_nan=True), on
        outs[on] = img
    assert np.isfinite(outs[True]).all() and not np.array_equal(outs[True], outs[False])
