"""JPEG output on the GPU: hhsr_jpeg_dct and hhsr_jpeg_entropy against the restatement tests/jpeg_ref.py, encode_jpeg's files,
and process() with output.format = jpeg.  The coefficients are compared under the near-tie rule below, everything after them
— scan bytes, length word, file — at tolerance 0.

Every device buffer a call writes (coefficients, scratch, scan, length word) lies between two 0xA5 guard bands of 256 bytes,
and the bands are checked after every call."""
import functools
import io

import numpy as np
import pytest
import torch

import jpeg_ref as ref

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, synthetic as synth, utils_image

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256
SHAPES = [(1, 1), (8, 8), (9, 17), (3, 64), (40, 72), (136, 264)]
QUALITIES = [50, 90, 100]
KINDS = ["random", "smooth", "constant", "wild"]
TIE = 0.004        # a float64 coefficient nearer than this to (n + 1/2) Q may round either way
TIE_SHARE = 0.04   # ... and at most this share of a case's coefficients is that near
B_RGB, B_GREY = 3, 2  # Pillow's decode vs ref.decode: measured 2 / 1 on the CPU (tests/test_jpeg_host.py), + 1


class Guarded:
    """n bytes of device memory between two guard bands, everything pre-filled with 0xA5."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self):
        """The n bytes, after checking that the bands still hold 0xA5."""
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == FILL).all() and (got[GUARD + self.n:] == FILL).all(), "a guard band was written"
        return got[GUARD:GUARD + self.n]


def gpu_dct(img, quality, och):
    """hhsr_jpeg_dct of a float32 ndarray -> int16 [n_mcu, och, 64]."""
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    coef_bytes, _, _ = utils_image.jpeg_workspace(H, W, och, 1)
    my, mx = ref.mcu_grid(H, W)
    assert coef_bytes == my * mx * och * 128
    out = Guarded(coef_bytes)
    src = torch.tensor(img).cuda()
    _lib.call("hhsr_jpeg_dct", _lib.ptr(src), H, W, ch, och, quality, out.ptr, coef_bytes, _lib.stream())
    return out.read().view(np.int16).reshape(my * mx, och, 64).copy()


def gpu_entropy(coef, H, W, ri, capacity=None):
    """hhsr_jpeg_entropy of an int16 ndarray -> (the first min(length, capacity) bytes of the scan, the length word, the
    whole scan buffer).  capacity None: the largest scan hhsr_jpeg_workspace states."""
    n_mcu, C, _ = coef.shape
    coef_bytes, scratch_bytes, bound = utils_image.jpeg_workspace(H, W, C, ri)
    assert coef_bytes == coef.nbytes
    cap = bound if capacity is None else capacity
    dev = torch.tensor(np.ascontiguousarray(coef, np.int16)).cuda()
    scratch, scan, length = Guarded(scratch_bytes), Guarded(cap), Guarded(8)
    _lib.call("hhsr_jpeg_entropy", _lib.ptr(dev), H, W, C, ri, scratch.ptr, scratch_bytes, scan.ptr, cap, length.ptr,
              _lib.stream())
    scratch.read()
    n = int(length.read().view(np.uint64)[0])
    whole = scan.read()
    return whole[:min(n, cap)].tobytes(), n, whole


@functools.lru_cache(maxsize=None)
def case(shape, channels, kind, quality):
    """(image, the GPU's coefficients, the float64 coefficients before the division) — computed once, read-only."""
    img = ref.test_images(shape[0], shape[1], channels, seed=shape[0] * 7 + shape[1] + channels)[kind]
    got = gpu_dct(img, quality, channels)
    co = ref.dct_unquantised(ref.samples(img))
    for a in (img, got, co):
        a.setflags(write=False)
    return img, got, co


@functools.lru_cache(maxsize=None)
def case_ac(shape, channels, kind, quality):
    return ref.ac_strings(case(shape, channels, kind, quality)[1])


def ids(s):
    return "%dx%d" % s


# ---- 1. coefficients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_coefficients_match_the_float64_restatement(shape, channels):
    """Equal, except where the float64 value lies within 0.004 of a rounding boundary: there the float32 transform may round
    the other way, by one.  (Budget: the float32 rounding of some 40 operations at magnitudes up to 1024.)"""
    for kind in KINDS:
        for quality in QUALITIES:
            img, got, co = case(shape, channels, kind, quality)
            want, tie = ref.quantise(co, quality)
            d = got.astype(int) - want.astype(int)
            near = tie < TIE
            share = float(near.mean())
            print(f"{ids(shape)} x {channels} {kind} q{quality}: {int((d != 0).sum())} of {d.size} differ, max |d| "
                  f"{int(np.abs(d).max())}, near-ties {100 * share:.2f} %, differing away from a tie {int((d != 0)[~near].sum())}")
            assert (d[~near] == 0).all(), (kind, quality, "a coefficient differs away from a rounding boundary")
            assert (np.abs(d) <= 1).all(), (kind, quality)
            assert share <= TIE_SHARE, (kind, quality, share)


def test_grey_file_of_an_rgb_image_takes_channel_0():
    img = ref.test_images(9, 17, 3, seed=5)["wild"]
    got = gpu_dct(img, 90, 1)
    assert np.array_equal(got, gpu_dct(np.ascontiguousarray(img[..., 0]), 90, 1))
    want, tie = ref.quantise(ref.dct_unquantised(ref.samples(img, 1)), 90)
    assert (got == want)[tie >= TIE].all() and np.abs(got.astype(int) - want).max() <= 1


# ---- 2. entropy coder on the GPU's own coefficients -------------------------------------------------------------------------------
def restarts(shape):
    my, mx = ref.mcu_grid(*shape)
    return sorted({1, 3, my * mx, 65535} | ({4} if shape == (40, 72) else set()))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_scan_matches_the_restated_coder(shape, channels):
    H, W = shape
    for kind in KINDS:
        for quality in QUALITIES:
            coef = case(shape, channels, kind, quality)[1]
            for ri in restarts(shape):
                want = ref.scan_bytes(coef, ri, ac=case_ac(shape, channels, kind, quality))
                got, n, _ = gpu_entropy(coef, H, W, ri)
                assert n == len(want), (kind, quality, ri, n, len(want))
                assert got == want, (kind, quality, ri)


def test_ri_4_on_45_mcus_wraps_the_marker_index():
    coef = case((40, 72), 3, "random", 100)[1]
    got, n, _ = gpu_entropy(coef, 40, 72, 4)
    marks = [got[i + 1] for i in range(len(got) - 1) if got[i] == 0xFF and got[i + 1] != 0]
    assert marks == [0xD0 + k % 8 for k in range(11)]  # 12 intervals, the last one short (1 MCU), no marker behind it


# ---- 3. entropy coder on hand-made coefficients -----------------------------------------------------------------------------------
def handmade(C):
    """{name: int16 [6 MCUs of a 16 x 24 image, C, 64]} — the places where Huffman coders break."""
    n = 6
    z = lambda: np.zeros((n, C, 64), np.int16)  # noqa: E731
    out = {"all_zero": z()}
    a = z(); a[:, :, 63] = [[5, -3, 1][:C]] * n; out["only_63"] = a                       # no EOB
    a = z()
    for m, run in enumerate((15, 16, 17, 32, 62, 47)):                                       # ZRL x 0, 1, 1, 2, 3, 2
        a[m, :, run + 1] = m + 1
        if run < 62:
            a[m, 0, 63] = -1 if m % 2 else 0                                                  # a second run behind it / EOB
    out["zero_runs"] = a
    a = z(); a[:, :, 1::2] = 1023; a[:, :, 2::2] = -1023
    a[0::2, :, 0], a[1::2, :, 0] = 1023, -1024                                              # DC steps of +-2047
    out["extremes"] = a
    a = z(); a[:, :, 0] = [[32767, -32768, 1024][:C], [-1025, 2000, -5000][:C]] * 3         # beyond the range: clamped
    a[:, :, 1:8] = [32767, -32768, 1024, -1024, 1023, -1023, 0]
    out["beyond_range"] = a
    a = z(); a[:, :, 0] = 255 * (np.arange(n)[:, None] % 2); a[:, :, 1:] = 1023              # magnitudes of 1-bits: 0xFF in the
    out["ones"] = a                                                                          # data and in the padded last byte
    a = z(); a[:, :, 0] = -np.arange(n)[:, None] * 100; a[:, :, 63] = 1023; a[:, :, 5] = 127
    out["ones_sparse"] = a
    rng = np.random.default_rng(11 + C)
    out["random_int16"] = rng.integers(-32768, 32768, (n, C, 64)).astype(np.int16)
    a = rng.integers(-3, 4, (n, C, 64)).astype(np.int16); a[rng.random((n, C, 64)) < 0.7] = 0
    out["sparse_small"] = a
    return out


@pytest.mark.parametrize("C", [1, 3])
def test_scan_of_handmade_coefficients(C):
    stuffed = padded_ff = False
    for name, coef in handmade(C).items():
        for ri in (1, 2, 4, 65535):
            want = ref.scan_bytes(coef, ri)
            got, n, _ = gpu_entropy(coef, 16, 24, ri)
            assert n == len(want) and got == want, (name, ri)
            stuffed |= b"\xFF\x00" in want
            padded_ff |= b"\xFF\x00\xFF\xD0" in want  # a padded last byte 0xFF, stuffed, then RST0
    assert stuffed and padded_ff, "the hand-made arrays no longer produce 0xFF bytes"


@pytest.mark.parametrize("C", [1, 3])
def test_scan_of_a_one_mcu_image(C):
    for name, coef in handmade(C).items():
        one = coef[1:2]
        for H, W in ((8, 8), (1, 1)):
            for ri in (1, 65535):
                want = ref.scan_bytes(one, ri)
                got, n, _ = gpu_entropy(one, H, W, ri)
                assert n == len(want) and got == want, (name, H, W, ri)


def test_an_interval_longer_than_one_pass_of_the_wave():
    """Ri = 30 MCUs of three components: 90 blocks, more than the 64 a wave codes at a time — bits carried between passes —
    and with the worst-case array every pass fills its bit buffer."""
    rng = np.random.default_rng(2)
    n = 9 * 33  # 72 x 264
    worst = np.full((n, 3, 64), -1023, np.int16)
    worst[:, :, 1::2] = 1023
    worst[0::2, :, 0], worst[1::2, :, 0] = -1024, 1023
    mixed = rng.integers(-40, 41, (n, 3, 64)).astype(np.int16)
    mixed[rng.random(mixed.shape) < 0.5] = 0
    for coef in (worst, mixed):
        ac = ref.ac_strings(coef)
        for ri in (30, 100, 65535):
            want = ref.scan_bytes(coef, ri, ac=ac)
            got, n_got, _ = gpu_entropy(coef, 72, 264, ri)
            assert n_got == len(want) and got == want, ri


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_is_never_exceeded():
    coef = case((40, 72), 3, "random", 100)[1]
    for ri in (4, 65535):
        want = ref.scan_bytes(coef, ri)
        need = len(want)
        got, n, whole = gpu_entropy(coef, 40, 72, ri, capacity=need)  # exactly enough
        assert n == need and got == want
        for cap in (need - 1, need // 2, 1, 0):                        # too small: the length is reported, the guards hold
            got, n, whole = gpu_entropy(coef, 40, 72, ri, capacity=cap)
            assert n == need and len(whole) == cap


def test_encode_jpeg_retries_once_with_the_reported_length(monkeypatch):
    img, coef, _ = case((40, 72), 3, "random", 100)
    want = ref.file_bytes(coef, 40, 72, 100, utils_image.JPEG_RESTART_MCUS)
    assert len(want) - 631 > 1000  # (measured: 12.4 kB of scan — the first guess below is exceeded)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    dev = torch.tensor(img).cuda()
    small = utils_image.encode_jpeg(dev, quality=100, capacity=1000)
    assert calls.count("hhsr_jpeg_entropy") == 2 and calls.count("hhsr_jpeg_dct") == 1
    del calls[:]
    full = utils_image.encode_jpeg(dev, quality=100)
    assert calls.count("hhsr_jpeg_entropy") == 1
    assert small.dtype == np.uint8 and small.ndim == 1 and small.tobytes() == full.tobytes() == want


# ---- 5. whole files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_files_are_the_restated_files_and_open_in_pillow(shape, channels, tmp_path):
    H, W = shape
    files = {}
    for kind in KINDS:
        for quality in QUALITIES:
            img, coef, _ = case(shape, channels, kind, quality)
            data = utils_image.encode_jpeg(torch.tensor(img).cuda(), quality=quality, restart_mcus=7)
            assert data.tobytes() == ref.file_bytes(coef, H, W, quality, 7), (kind, quality)
            files[kind, quality] = data
    utils_image.save_jpeg(files["smooth", 90], str(tmp_path / "a.jpg"))
    assert (tmp_path / "a.jpg").read_bytes() == files["smooth", 90].tobytes()
    Image = pytest.importorskip("PIL.Image")
    worst = 0
    for (kind, quality), data in files.items():
        im = Image.open(io.BytesIO(data.tobytes()))
        im.load()
        assert im.size == (W, H) and im.mode == ("L" if channels == 1 else "RGB")
        want = ref.decode(case(shape, channels, kind, quality)[1], H, W, quality)
        worst = max(worst, int(np.abs(np.asarray(im).astype(int) - want.astype(int)).max()))
    print(f"Pillow vs restated decode of the GPU's coefficients, {channels} channel(s), {H}x{W}: max {worst}")
    assert worst <= (B_GREY if channels == 1 else B_RGB)


# ---- 6. reproducibility -----------------------------------------------------------------------------------------------------------
def test_bytes_are_reproducible_and_stream_independent():
    img = case((136, 264), 3, "smooth", 90)[0]
    dev = torch.tensor(img).cuda()
    a = utils_image.encode_jpeg(dev, quality=90, restart_mcus=3)
    b = utils_image.encode_jpeg(dev, quality=90, restart_mcus=3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = utils_image.encode_jpeg(dev, quality=90, restart_mcus=3)
    side.synchronize()
    assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- 7. process() -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def burst():
    ref_raw, comp, _ = synth.make_burst(128, 160, 3, seed=21, max_shift=1.5)
    std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    return {"ref": ref_raw, "comp": comp, "cfa_pattern": np.array([[0, 1], [1, 2]]), "white_balance": np.ones(3),
            "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "std_curve": std, "diff_curve": diff, "orientation": 6}


def config(output, mode="bayer"):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.scale = 2
    cfg.mode = mode
    cfg.block_matching.tuning.tile_size = 16
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg.block_matching.tuning.metrics = ["L2"] * 4
    cfg.robustness.save_mask = True
    if output is not None:
        cfg.output = dict(output)
    return cfg


@functools.lru_cache(maxsize=None)
def processed(output, mode="bayer"):
    """process() of the burst at x2, once per configuration; `output`: the items of config.output, or None for no section."""
    return hsr.process(dict(burst()), config(None if output is None else dict(output), mode))


def sof_components(data):
    i = data.tobytes().index(b"\xFF\xC0")
    return int(data[i + 9]), (int(data[i + 5]) << 8 | int(data[i + 6]), int(data[i + 7]) << 8 | int(data[i + 8]))


def test_process_returns_the_file():
    f32, _ = processed(None)
    u8, dbg8 = processed((("dtype", "uint8"),))
    jpg, dbg = processed((("format", "jpeg"), ("quality", 85), ("restart_mcus", 16)))
    assert f32.dtype == np.float32 and f32.shape == (320, 256, 3)
    assert jpg.dtype == np.uint8 and jpg.ndim == 1 and sof_components(jpg) == (3, (320, 256))
    want = utils_image.encode_jpeg(torch.tensor(f32).cuda(), quality=85, restart_mcus=16)
    assert jpg.tobytes() == want.tobytes()
    assert jpg.size < u8.size // 3                              # (what the format is for)
    assert dbg["robustness mask"].dtype == np.uint8 and np.array_equal(dbg["robustness mask"], dbg8["robustness mask"])
    assert dbg["accumulated robustness"].tobytes() == dbg8["accumulated robustness"].tobytes()
    dflt, _ = processed((("format", "jpeg"), ("dtype", "uint8")))  # quality 90, the default interval
    assert dflt.tobytes() == utils_image.encode_jpeg(torch.tensor(f32).cuda()).tobytes()
    assert dflt[:623].tobytes() == ref.header(320, 256, 3, 90, utils_image.JPEG_RESTART_MCUS)[:623]


def test_process_grey_mode_is_one_component():
    f32, _ = processed(None, "grey")
    jpg, _ = processed((("format", "jpeg"),), "grey")
    assert np.isnan(f32[..., 1:]).all() and sof_components(jpg) == (1, (320, 256))
    assert jpg.tobytes() == utils_image.encode_jpeg(torch.tensor(f32).cuda(), channels=1).tobytes()


def test_process_without_the_format_key_is_unchanged():
    f32, d32 = processed(None)
    for out in ((("format", "raw"),), (("format", "raw"), ("dtype", "float32"))):
        got, dbg = processed(out)
        assert got.dtype == np.float32 and got.tobytes() == f32.tobytes() and sorted(dbg) == sorted(d32)
    u8, d8 = processed((("dtype", "uint8"),))
    got, dbg = processed((("dtype", "uint8"), ("format", "raw")))
    assert got.dtype == np.uint8 and got.shape == (320, 256, 3) and got.tobytes() == u8.tobytes()
    assert np.array_equal(u8, ref.samples(f32)) and np.array_equal(dbg["robustness mask"], d8["robustness mask"])


@pytest.mark.parametrize("output", [{"format": "jpeg", "dtype": "uint16"}, {"format": "jpeg", "dtype": "float32"},
                                    {"format": "jpg"}, {"format": "jpeg", "quality": 0}, {"format": "jpeg", "restart_mcus": 0}])
def test_process_refuses_contradictions(output):
    with pytest.raises(ValueError):
        hsr.process(dict(burst()), config(output))
