"""Extended JPEG output on the GPU: 4:2:0 coefficients, the generalised entropy coder, the symbol histogram, optimised tables,
encode_jpeg's new options and process() with them, against the restatement tests/jpeg_ex_ref.py.  Coefficients are compared
under the near-tie rule of tests/test_jpeg_encode.py, everything after them at tolerance 0.

Every device buffer a call writes lies between two 0xA5 guard bands of 256 bytes (test_jpeg_encode.Guarded)."""
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_ex_ref as ex
import jpeg_ref as ref
import test_jpeg_encode as base
from test_jpeg_ex_host import all_symbols_fibonacci

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, utils_image

pytestmark = pytest.mark.gpu

Guarded, TIE, TIE_SHARE, KINDS, QUALITIES, ids = base.Guarded, base.TIE, base.TIE_SHARE, base.KINDS, base.QUALITIES, base.ids
# 24 x 520: 33 MCUs across, a partial MCU more than the 16 MCUs x 2 of two DCT workgroups
SHAPES = [(1, 1), (16, 16), (17, 33), (9, 17), (3, 64), (40, 72), (136, 264), (24, 520)]
U64_MAX = (1 << 64) - 1


def gpu_dct_ex(img, quality, och, sub):
    """hhsr_jpeg_dct_ex of a float32 ndarray -> int16 [n_mcu, blocks per MCU, 64]."""
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    coef_bytes, _, _ = utils_image.jpeg_workspace_ex(H, W, och, 1, sub)
    my, mx = ex.mcu_grid(H, W, sub)
    bpm = 6 if sub else och
    assert coef_bytes == my * mx * bpm * 128
    out = Guarded(coef_bytes)
    src = torch.tensor(img).cuda()
    _lib.call("hhsr_jpeg_dct_ex", _lib.ptr(src), H, W, ch, och, quality, sub, out.ptr, coef_bytes, _lib.stream())
    return out.read().view(np.int16).reshape(my * mx, bpm, 64).copy()


def spec_ptr(spec):
    return None if spec is None else utils_image._jpeg_spec(spec, spec.shape[0])


def gpu_entropy_ex(coef, H, W, och, ri, sub, spec=None, capacity=None):
    """hhsr_jpeg_entropy_ex -> (the first min(length, capacity) bytes of the scan, the length word, the whole buffer)."""
    _, scratch_bytes, _, bound = ex.workspace(H, W, och, ri, sub)
    assert coef.nbytes == ex.workspace(H, W, och, ri, sub)[0]
    cap = bound if capacity is None else capacity
    dev = torch.tensor(np.ascontiguousarray(coef, np.int16)).cuda()
    scratch, scan, length = Guarded(scratch_bytes), Guarded(cap), Guarded(8)
    _lib.call("hhsr_jpeg_entropy_ex", _lib.ptr(dev), H, W, och, ri, sub, spec_ptr(spec), scratch.ptr, scratch_bytes, scan.ptr,
              cap, length.ptr, _lib.stream())
    scratch.read()
    n = int(length.read().view(np.uint64)[0])
    whole = scan.read()
    return whole[:min(n, cap)].tobytes(), n, whole


def gpu_histogram(coef, H, W, och, sub, ri, counts=None):
    """hhsr_jpeg_histogram -> uint64 [4, 256]; `counts`: a Guarded buffer to count into again."""
    _, _, scratch_bytes, _ = ex.workspace(H, W, och, ri, sub)
    dev = torch.tensor(np.ascontiguousarray(coef, np.int16)).cuda()
    scratch = Guarded(scratch_bytes)
    counts = Guarded(8192) if counts is None else counts
    _lib.call("hhsr_jpeg_histogram", _lib.ptr(dev), H, W, och, sub, ri, counts.ptr, scratch.ptr, scratch_bytes, _lib.stream())
    scratch.read()
    return counts.read().view(np.uint64).reshape(4, 256).copy()


@functools.lru_cache(maxsize=None)
def case(shape, kind, quality):
    """(image, the GPU's 4:2:0 coefficients, the float64 coefficients before the division) — computed once, read-only."""
    img = ref.test_images(shape[0], shape[1], 3, seed=shape[0] * 7 + shape[1] + 3)[kind]
    got = gpu_dct_ex(img, quality, 3, 1)
    co = ex.dct_unquantised_420(ref.samples(img))
    for a in (img, got, co):
        a.setflags(write=False)
    return img, got, co


def restarts(shape):
    my, mx = ex.mcu_grid(*shape, 1)
    return sorted({1, 3, 11, 30, my * mx, 65535})


def handmade420():
    """The hand-made arrays of test_jpeg_encode.handmade(3), two MCUs of three blocks each rebuilt as one of six: [3, 6, 64]
    for a 16 x 48 image."""
    return {name: a.reshape(3, 6, 64) for name, a in base.handmade(3).items()}


# ---- 1. coefficients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_420_coefficients_match_the_float64_restatement(shape):
    """Equal, except where the float64 value lies within 0.004 of a rounding boundary: there the float32 transform may round
    the other way, by one (the rule and the budget of tests/test_jpeg_encode.py; the box filter adds three float32 additions
    and an exact multiplication in front of the transform)."""
    for kind in KINDS:
        for quality in QUALITIES:
            _, got, co = case(shape, kind, quality)
            want, tie = ex.quantise_420(co, quality)
            d = got.astype(int) - want.astype(int)
            near = tie < TIE
            share = float(near.mean())
            print(f"{ids(shape)} {kind} q{quality}: {int((d != 0).sum())} of {d.size} differ, max |d| {int(np.abs(d).max())}, "
                  f"near-ties {100 * share:.2f} %, differing away from a tie {int((d != 0)[~near].sum())}")
            assert (d[~near] == 0).all(), (kind, quality, "a coefficient differs away from a rounding boundary")
            assert (np.abs(d) <= 1).all(), (kind, quality)
            assert share <= TIE_SHARE, (kind, quality, share)


# ---- 2. Y is today's Y ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_y_blocks_are_the_444_y_blocks_bit_for_bit(shape):
    H, W = shape
    for kind in KINDS:
        for quality in QUALITIES:
            img, got, _ = case(shape, kind, quality)
            y, have = ex.y_of_444(base.gpu_dct(img, quality, 3), H, W)
            assert have.any() and np.array_equal(got[:, :4][have], y[have]), (kind, quality)


# ---- 3. the standard-table scan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_420_scan_matches_the_restated_coder(shape):
    H, W = shape
    for kind, quality in [(k, 90) for k in KINDS] + [("random", 100), ("smooth", 50)]:
        coef = case(shape, kind, quality)[1]
        for ri in restarts(shape):
            want = ex.scan_bytes(coef, ri, 1)
            got, n, _ = gpu_entropy_ex(coef, H, W, 3, ri, 1)
            assert n == len(want), (kind, quality, ri, n, len(want))
            assert got == want, (kind, quality, ri)


def test_420_scan_of_handmade_coefficients():
    stuffed = False
    for name, coef in handmade420().items():
        for ri in (1, 2, 65535):
            want = ex.scan_bytes(coef, ri, 1)
            got, n, _ = gpu_entropy_ex(coef, 16, 48, 3, ri, 1)
            assert n == len(want) and got == want, (name, ri)
            stuffed |= b"\xFF\x00" in want
        one = coef[1:2]  # a one-MCU image
        for H, W in ((16, 16), (1, 1)):
            for ri in (1, 65535):
                want = ex.scan_bytes(one, ri, 1)
                got, n, _ = gpu_entropy_ex(one, H, W, 3, ri, 1)
                assert n == len(want) and got == want, (name, H, W, ri)
    assert stuffed


# ---- 4. (0, NULL) is the old entry points ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_ex_with_defaults_equals_the_old_entry_points(channels):
    for shape in ((9, 17), (40, 72), (136, 264)):
        H, W = shape
        for kind in KINDS:
            img = ref.test_images(H, W, channels, seed=H + W + channels)[kind]
            for och in {channels, 1}:
                old = base.gpu_dct(img, 90, och)
                assert np.array_equal(old, gpu_dct_ex(img, 90, och, 0)), (shape, kind, och)
                for ri in (1, 4, 30, 65535):
                    a, na, _ = base.gpu_entropy(old, H, W, ri)
                    b, nb, _ = gpu_entropy_ex(old, H, W, och, ri, 0)
                    assert na == nb and a == b, (shape, kind, och, ri)


# ---- 5. histogram ---------------------------------------------------------------------------------------------------------------
def check_histogram(coef, H, W, channels, sub):
    n_mcu = coef.shape[0]
    buf = Guarded(8192)
    for ri in sorted({1, 3, 11, 30, n_mcu, 65535}):
        want = ex.histogram(coef, ri, sub)
        got = gpu_histogram(coef, H, W, channels, sub, ri, buf)  # the same buffer every time: overwritten, not added to
        assert np.array_equal(got, want), (sub, channels, ri)
        assert np.array_equal(gpu_histogram(coef, H, W, channels, sub, ri, buf), want), "a second call differs"
        assert channels == 3 or not got[2:].any()


@pytest.mark.parametrize("shape", [(17, 33), (40, 72), (136, 264), (24, 520)], ids=ids)
def test_histogram_of_420_equals_the_restated_counts(shape):
    for kind in ("random", "smooth", "wild"):
        check_histogram(case(shape, kind, 90)[1], *shape, 3, 1)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", [(9, 17), (136, 264)], ids=ids)
def test_histogram_of_444_equals_the_restated_counts(shape, channels):
    for kind in ("random", "smooth", "wild"):
        check_histogram(base.case(shape, channels, kind, 90)[1], *shape, channels, 0)


# ---- 6. optimised files ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_optimised_files_are_the_restated_files(shape):
    Image = pytest.importorskip("PIL.Image")
    H, W = shape
    for kind, quality, ri in (("random", 100, 65535), ("smooth", 90, 4), ("wild", 50, 1), ("constant", 90, 3)):
        img, coef, _ = case(shape, kind, quality)
        dev = torch.tensor(img).cuda()
        specs = ex.huffman_specs(ex.histogram(coef, ri, 1), 3)
        want = ex.file_bytes(coef, H, W, quality, ri, 1, specs)
        got = utils_image.encode_jpeg(dev, quality=quality, restart_mcus=ri, subsampling="420", huffman="optimized")
        assert got.tobytes() == want, (kind, quality, ri)
        std = utils_image.encode_jpeg(dev, quality=quality, restart_mcus=ri, subsampling=420)
        assert std.tobytes() == ex.file_bytes(coef, H, W, quality, ri, 1), (kind, quality, ri)
        assert got.size - len(ex.header(H, W, 3, quality, ri, 1, specs)) <= std.size - len(ex.header(H, W, 3, quality, ri, 1))
        a, b = (np.asarray(Image.open(io.BytesIO(d.tobytes()))) for d in (got, std))
        assert a.shape == (H, W, 3) and np.array_equal(a, b), "the optimised file decodes to other pixels"


def test_optimised_444_files_are_the_restated_files():
    for channels in (1, 3):
        img, coef, _ = base.case((40, 72), channels, "smooth", 90)
        specs = ex.huffman_specs(ex.histogram(coef, 7), channels)
        got = utils_image.encode_jpeg(torch.tensor(img).cuda(), quality=90, restart_mcus=7, huffman="optimized")
        assert got.tobytes() == ex.file_bytes(coef, 40, 72, 90, 7, 0, specs)
        assert got.size < len(ref.file_bytes(coef, 40, 72, 90, 7))


# ---- 7. a length-limited specification ------------------------------------------------------------------------------------------
def test_length_limited_tables_code_every_symbol():
    counts = all_symbols_fibonacci()
    assert max(ex.code_lengths(counts[1]).values()) > 16
    specs = ex.huffman_specs(counts, 3)
    assert max(i + 1 for i, b in enumerate(specs[1][0]) if b) == 16 and len(specs[1][1]) == 162 and len(specs[0][1]) == 12
    arr = ex.spec_array(specs)
    for sub, coef, (H, W) in ((1, handmade420()["random_int16"], (16, 48)), (0, base.handmade(3)["random_int16"], (16, 24))):
        for ri in (1, 2, 65535):
            want = ex.scan_bytes(coef, ri, sub, specs)
            got, n, _ = gpu_entropy_ex(coef, H, W, 3, ri, sub, arr)
            assert want is not None and n == len(want) and got == want, (sub, ri)


# ---- 8. a missing symbol --------------------------------------------------------------------------------------------------------
def test_a_missing_symbol_is_reported_in_the_length_word():
    coef = np.zeros((3, 6, 64), np.int16)
    coef[:, :4, 0], coef[:, 4:, 0] = 500, 501  # at Ri = 1 every difference is 500, 3 x 0 | 501: categories 9 and 0
    specs = ex.huffman_specs(ex.histogram(coef, 1, 1), 3)
    arr = ex.spec_array(specs)
    want = ex.scan_bytes(coef, 1, 1, specs)
    got, n, _ = gpu_entropy_ex(coef, 16, 48, 3, 1, 1, arr)
    assert n == len(want) and got == want
    assert ex.scan_bytes(coef, 65535, 1, specs) is None  # Cb / Cr of the second MCU: difference 0, and no such code
    _, n, _ = gpu_entropy_ex(coef, 16, 48, 3, 65535, 1, arr)  # (the guard bands are checked in there)
    assert n == U64_MAX
    _, n, whole = gpu_entropy_ex(coef, 16, 48, 3, 65535, 1, arr, capacity=3)
    assert n == U64_MAX and len(whole) == 3


# ---- 9. capacity ------------------------------------------------------------------------------------------------------------------
def test_420_capacity_is_never_exceeded():
    img, coef, _ = case((40, 72), "random", 100)
    for ri in (4, 65535):
        arr = ex.spec_array(ex.huffman_specs(ex.histogram(coef, ri, 1), 3))
        want = ex.scan_bytes(coef, ri, 1, ex.huffman_specs(ex.histogram(coef, ri, 1), 3))
        need = len(want)
        got, n, _ = gpu_entropy_ex(coef, 40, 72, 3, ri, 1, arr, capacity=need)
        assert n == need and got == want
        for cap in (need - 1, 0):
            _, n, whole = gpu_entropy_ex(coef, 40, 72, 3, ri, 1, arr, capacity=cap)
            assert n == need and len(whole) == cap
    dev = torch.tensor(img).cuda()
    small = utils_image.encode_jpeg(dev, quality=100, capacity=100, subsampling="420", huffman="optimized")
    assert small.tobytes() == utils_image.encode_jpeg(dev, quality=100, subsampling="420", huffman="optimized").tobytes()


# ---- 10. process() ----------------------------------------------------------------------------------------------------------------
def test_process_with_420_and_optimised_tables():
    f32, _ = base.processed(None)
    jpg, _ = base.processed((("format", "jpeg"), ("subsampling", 420), ("huffman", "optimized")))
    dflt, _ = base.processed((("format", "jpeg"), ("dtype", "uint8")))
    want = utils_image.encode_jpeg(torch.tensor(f32).cuda(), subsampling="420", huffman="optimized")
    assert jpg.dtype == np.uint8 and jpg.ndim == 1 and jpg.tobytes() == want.tobytes()
    assert ex.sof_factors(jpg) == [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)] and base.sof_components(jpg) == (3, (320, 256))
    assert jpg.size < dflt.size
    text, _ = base.processed((("format", "jpeg"), ("subsampling", "420"), ("huffman", "optimized")))
    assert text.tobytes() == jpg.tobytes()
    ignored, _ = base.processed((("dtype", "uint8"), ("subsampling", "nonsense")))  # read only with format: jpeg
    assert ignored.dtype == np.uint8 and ignored.shape == (320, 256, 3)


@pytest.mark.parametrize("output,mode", [({"format": "jpeg", "subsampling": "422"}, "bayer"),
                                         ({"format": "jpeg", "subsampling": 411}, "bayer"),
                                         ({"format": "jpeg", "huffman": "optimised"}, "bayer"),
                                         ({"format": "jpeg", "huffman": 1}, "bayer"),
                                         ({"format": "jpeg", "subsampling": 420}, "grey"),
                                         ({"format": "jpeg", "subsampling": "420", "huffman": "optimized"}, "grey")])
def test_process_refuses_the_new_contradictions(output, mode):
    with pytest.raises(ValueError):
        hsr.process(dict(base.burst()), base.config(output, mode))


# ---- 11. reproducibility --------------------------------------------------------------------------------------------------------
def test_420_optimised_bytes_are_reproducible_and_stream_independent():
    dev = torch.tensor(case((136, 264), "smooth", 90)[0]).cuda()
    kw = dict(quality=90, restart_mcus=3, subsampling="420", huffman="optimized")
    a = utils_image.encode_jpeg(dev, **kw)
    b = utils_image.encode_jpeg(dev, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = utils_image.encode_jpeg(dev, **kw)
    side.synchronize()
    assert a.tobytes() == b.tobytes() == c.tobytes()
