"""The tone-mapping contract without a GPU: properties of its NumPy restatement (tests/mertens_ref.py: OpenCV 4.x
MergeMertens restated operation by operation; never compared with a cv2 run, PARITY.md) and the host-only parts of the
library (workspace query, argument refusals).

Measured on the CPU (figures in PARITY.md): partition of unity <= 2.4e-7; float32 against float64 blend 2.4e-7 - 4.8e-7;
output shift on the exactly-grey region when the channel mean is computed as / 3: 0.30."""
import ctypes

import numpy as np
import pytest

import mertens_ref as ref
from tonemap_cases import EPS32, F32, SHAPES, blend_bound, case, image, log_figure, regions


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 13, 37])
def test_pyr_down_is_the_mirrored_binomial_filter(n):
    """pyr_down = scipy.ndimage.correlate1d([1 4 6 4 1] / 16, mode="mirror") sampled at 2 i, per axis — down to axis
    lengths 1, 2 and 3, where the reflection is applied more than once."""
    from scipy.ndimage import correlate1d

    rng = np.random.default_rng(n)
    k = np.array([1, 4, 6, 4, 1]) / 16.0
    for shape in ((n, 11), (11, n), (n, n)):
        a = rng.random(shape)
        want = correlate1d(correlate1d(a, k, axis=1, mode="mirror"), k, axis=0, mode="mirror")[::2, ::2]
        got = ref.pyr_down(a)
        assert got.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
        assert np.abs(got - want).max() < 1e-14, shape


def test_pyr_up_interpolates_and_crops():
    """A constant stays constant at both parities of the size, the odd size is the even one without its last sample,
    and the taps are (1 6 1) / 8 and (1 1) / 2 with s[-1] = s[1], s[n] = s[n - 1]."""
    s = np.full((3, 4), 0.7)
    assert np.allclose(ref.pyr_up(s, (6, 8)), 0.7, atol=1e-15) and np.allclose(ref.pyr_up(s, (5, 7)), 0.7, atol=1e-15)
    a = np.random.default_rng(0).random((4, 5))
    assert np.array_equal(ref.pyr_up(a, (8, 10))[:7, :9], ref.pyr_up(a, (7, 9)))
    r = np.array([[1.0, 2.0, 4.0]])
    assert np.allclose(ref.pyr_up(r, (1, 6))[0], [(2 + 6 + 2) / 8, 1.5, (1 + 12 + 4) / 8, 3, (2 + 24 + 4) / 8, 4], atol=1e-15)
    assert np.array_equal(ref.pyr_up(np.array([[3.0]]), (1, 1)), [[3.0]])  # n = 1: s[-1] = s[0]


def test_level_count_table():
    """L = floor(log2(min(H, W))) for every min = 1 ... 8192, powers of two included.  OpenCV's float32 expression
    int(logf(float(m)) / logf(2.f)) is the same table wherever its quotient is not within a rounding of an integer:
    away from powers of two always, at a power of two 2^k it gives k or k - 1 depending on the platform's logf (a
    correctly rounded logf gives 12 at 8192, PARITY.md)."""
    for m in range(1, 8193):
        k = m.bit_length() - 1
        assert ref.levels(m, 9000) == ref.levels(9000, m) == k, m
        f = ref.levels_float32(m)
        assert f == k or (m == 1 << k and f == k - 1), (m, f)


@pytest.mark.parametrize("shape", SHAPES)
def test_partition_of_unity(shape):
    """n identical exposures fuse to the exposure itself."""
    c = case(shape)
    L = ref.levels(*shape)
    worst = 0.0
    for n in (1, 3, 4):
        e = np.stack([c["expo"][0]] * n)
        got, wn = ref.mertens(e, smooth=False)
        assert np.abs(wn - 1.0 / n).max() <= EPS32  # w / ((w + w) + w): two roundings
        worst = max(worst, float(np.abs(got - ref.to_float(e[0])).max()))
    log_figure(f"restatement: n identical exposures vs the exposure, {shape}", worst, blend_bound(L), c["r32"].size)
    assert worst <= blend_bound(L)


@pytest.mark.parametrize("shape", SHAPES)
def test_float32_blend_against_float64(shape):
    """The float32 pyramids agree with float64 ones on the same float32 weights: the spread the GPU tests scale."""
    c = case(shape)
    bound = blend_bound(ref.levels(*shape))
    log_figure(f"restatement: float32 vs float64 blend, {shape}", c["spread"], bound, c["r32"].size)
    log_figure(f"restatement: float32 vs float64 blend + smoothstep, {shape}", c["spread_smooth"], 1.5 * bound, c["r32"].size)
    assert c["spread"] <= bound
    assert c["spread_smooth"] <= 1.5 * bound  # |d smoothstep / dr| <= 1.5


def test_flat_regions_have_the_floor_weight():
    """Contrast is an exact 0 where the five samples are equal, so every weight there is exactly 1e-12f — and the
    normalised weight exactly 1 / n."""
    H, W = 37, 53
    c = case((H, W))
    _, flat = regions(H, W)
    inner = np.zeros_like(flat)
    inner[1:-1, 1:-1] = flat[1:-1, 1:-1] & flat[:-2, 1:-1] & flat[2:, 1:-1] & flat[1:-1, :-2] & flat[1:-1, 2:]
    inner[-1, 1:W // 2 - 1] = True  # bottom border row: reflect-101 stays inside the flat region
    assert inner.sum() > 100
    w = ref.weight_maps(c["I"])
    assert (w[:, inner] == F32(1e-12)).all()
    assert (c["wn"][:, inner] == F32(1) / F32(3)).all()


def test_grey_pixels_are_decided_by_rounding():
    """On pixels with r = g = b the saturation is 0 or one rounding error, depending on how the channel mean is
    rounded: computing it as sum / 3 instead of sum * (1 / 3) changes the weights there and moves the fused image.
    The shift on the exactly-grey textured region is measured and logged (PARITY.md); a coloured region only moves
    through the pyramids' bleed from its neighbours."""
    H, W = 64, 96
    img = image(H, W, seed=1)
    grey, _ = regions(H, W)
    e = ref.exposures(img)
    assert (e[..., 0] == e[..., 1])[:, grey].all() and (e[..., 1] == e[..., 2])[:, grey].all()
    I = ref.to_float(e)
    w_mul, w_div = ref.weight_maps(I, "mul"), ref.weight_maps(I, "div")
    assert (w_mul[:, grey] < 1e-6).all() and (w_div[:, grey] < 1e-6).all()  # contrast x (0 or ~1 ulp) + 1e-12
    assert (w_mul[:, grey] != w_div[:, grey]).any()
    colour = np.zeros_like(grey)
    colour[:, W // 2 + 16:] = True  # 16 pixels away from the grey and flat halves
    assert np.array_equal(w_mul[:, colour], w_div[:, colour]) or np.abs(w_mul - w_div)[:, colour].max() < 1e-6
    a, b = ref.mertens(e, smooth=False, mean="mul")[0], ref.mertens(e, smooth=False, mean="div")[0]
    d = np.abs(a - b).max(-1)
    log_figure("restatement: fused shift on the grey region, channel mean as / 3", float(d[grey].max()), 1.0, int(grey.sum()))
    log_figure("restatement: fused shift on the coloured region, channel mean as / 3", float(d[colour].max()), 1.0, int(colour.sum()))
    assert d[grey].max() > 100 * blend_bound(ref.levels(H, W))  # far outside anything a tolerance could absorb


def test_exposures_are_not_clipped_first():
    """clip(1.5 x 0.5) = 0.75, not 0.5; rounding is half to even; float64 images keep float64 arithmetic."""
    img = np.array([[[1.5, -0.3, 0.5]]], F32)
    e = ref.exposures(img)
    assert e[:, 0, 0].tolist() == [[255, 0, 128], [191, 0, 64], [255, 0, 255]]  # 127.5 -> 128, 191.25 -> 191, 63.75 -> 64
    assert ref.exposures(np.array([[[2.5 / 255, 0.5 / 255, 1.5 / 255]]]))[0, 0, 0].tolist() == [2, 0, 2]


# ---- the library without a GPU ----------------------------------------------------------------------------------------
def _lib():
    from handheld_super_resolution import _lib

    return _lib.load()


def _workspace(lib, H, W, n):
    b, l = ctypes.c_size_t(0), ctypes.c_int(-1)
    rc = lib.hhsr_tonemap_workspace(H, W, n, ctypes.byref(b), ctypes.byref(l))
    return rc, b.value, l.value


def test_workspace_query_levels_and_bytes():
    lib = _lib()
    for shape in SHAPES + [(6000, 8000), (3000, 4000)]:
        rc, nbytes, lv = _workspace(lib, *shape, 3)
        assert rc == 0 and lv == ref.levels(*shape) and nbytes >= 4 * 3 * shape[0] * shape[1], shape
    for m in range(1, 8193):  # the float32 level count of the library's host code = the restatement's
        assert _workspace(lib, m, 8192, 1)[2] == m.bit_length() - 1, m
    sizes = sorted(SHAPES + [(100, 100), (101, 100), (1000, 1000)], key=lambda s: s[0] * s[1])
    got = [_workspace(lib, h, w, 3)[1] for h, w in sizes]
    assert got == sorted(got) and len(set(got)) > 1  # monotone in H W
    assert _workspace(lib, 37, 53, 4)[1] > _workspace(lib, 37, 53, 3)[1] > _workspace(lib, 37, 53, 1)[1]


def test_argument_refusals_do_not_touch_the_gpu():
    """Null pointers, sizes <= 0, n out of range, aliasing and a short workspace return -1 before any HIP call."""
    lib = _lib()
    V = ctypes.c_void_p
    b, l = ctypes.c_size_t(0), ctypes.c_int(0)
    for args in ((0, 8, 3), (8, -1, 3), (8, 8, 0), (8, 8, 5), (40000, 40000, 3)):
        assert lib.hhsr_tonemap_workspace(*args, ctypes.byref(b), ctypes.byref(l)) == -1, args
        assert b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_tonemap_workspace(8, 8, 3, None, ctypes.byref(l)) == -1
    assert lib.hhsr_tonemap_workspace(8, 8, 3, ctypes.byref(b), None) == -1

    H, W, n = 8, 8, 3
    _, need, _ = _workspace(lib, H, W, n)
    # fake, well separated device addresses: every call below is refused before a kernel could see them
    expo, work, out, wts = 0x10000000, 0x20000000, 0x30000000, 0x40000000

    def mertens(e=expo, n_=n, h=H, w=W, ws=work, nb=need, wo=wts, o=out):
        return lib.hhsr_mertens(V(e), n_, h, w, V(ws), nb, V(wo), V(o), 1, None)

    for kw in (dict(e=0), dict(ws=0), dict(o=0), dict(n_=0), dict(n_=5), dict(h=0), dict(w=-3), dict(nb=need - 1), dict(nb=0),
               dict(o=expo), dict(ws=expo), dict(o=work), dict(o=work + need - 4), dict(wo=out), dict(wo=work), dict(wo=expo + 4),
               dict(ws=work + 1), dict(h=40000, w=40000)):
        assert mertens(**kw) == -1, kw
        assert b"invalid argument" in lib.hhsr_last_error()

    img, tmp, taps = 0x50000000, 0x60000000, 0x70000000
    times = (ctypes.c_double * 3)(1.0, 0.5, 2.0)

    def expose(i=img, t=tmp, h=H, w=W, sharpen=0, tp=taps, radius=2, tm=times, n_=3, e=expo):
        return lib.hhsr_post_expose(V(i), V(t), h, w, None, sharpen, 0.5, V(tp), radius, 0, tm, n_, V(e), None)

    for kw in (dict(i=0), dict(e=0), dict(tm=None), dict(h=0), dict(w=0), dict(n_=0), dict(n_=5), dict(e=img), dict(e=tmp),
               dict(sharpen=1, t=0), dict(sharpen=1, tp=0), dict(sharpen=1, radius=65), dict(sharpen=1, radius=-1),
               dict(sharpen=1, t=img), dict(h=40000, w=40000)):
        assert expose(**kw) == -1, kw
        assert b"invalid argument" in lib.hhsr_last_error()
