"""Noise profile of a burst that brings none: without a GPU the NumPy restatement's accuracy on a texture-free scene, the
white-balance gains, the library's host fit against the NumPy fit, every refusal and the option checks of process(); on the
GPU hhsr_noise_profile_hist against the restatement bit for bit (strides, alignments, CFAs, batches, orders), the tile rules
by hand, graph capture, and process() with noise_model.source = estimate end to end."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import noise_profile_ref as ref

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, noise_profile as npf, utils_dng, synthetic as synth

RGGB, GRBG = [[0, 1], [1, 2]], [[1, 0], [2, 1]]
CFAS = {"rggb": RGGB, "grbg": GRBG, "mono": None}
A100, B100 = synth.ALPHA_ISO100, synth.BETA_ISO100
PROFILES = {"iso100": (A100, B100), "high": (16 * A100, 256 * B100)}
SEEDS = range(8)
# Largest relative error of sqrt(alpha x + beta) over x = 0.1 .. 0.9 on the smooth 512 x 768 scene, eight seeds: measured
# with the restatement of this repository 7.24 % (iso100) and 4.94 % (high); asserted: twice the worst, because eight seeds
# bound the tail loosely (PARITY.md "Noise profile")
MEASURED_WORST = 0.0724
BOUND = 2 * MEASURED_WORST
# the kernel's tiling (csrc/hhsr_noise_profile.hip): a workgroup covers NP_SPAN_BLOCKS = 32 blocks of 16 x 16 pixels
SPAN = 32 * 16
SHAPES = [(16, 16), (14, 40), (34, 50), (48, 80), (64, 2 * SPAN + 16)]  # the last: two workgroups plus one tile = 64 x 1040


# ---- without a GPU ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smooth_hist(profile, seed, wb=(1.0, 1.0, 1.0)):
    """Histogram of the noisy smooth scene (RGGB), multiplied per colour by `wb` after the clip."""
    a, b = PROFILES[profile]
    f = ref.noisy(ref.smooth_scene(512, 768), a, b, seed)
    f = apply_wb(f, RGGB, wb)
    h = ref.histogram([f], RGGB, wb)
    h.setflags(write=False)
    return h


def apply_wb(frame, cfa, wb):
    f = frame.copy()
    for p in range(4):
        f[p >> 1::2, p & 1::2] *= np.float32(wb[cfa[p >> 1][p & 1]] / wb[1])
    return f


@pytest.mark.parametrize("profile", list(PROFILES))
def test_restatement_accuracy_on_the_smooth_scene(profile):
    a0, b0 = PROFILES[profile]
    errs = []
    for seed in SEEDS:
        r = ref.fit(smooth_hist(profile, seed), RGGB)
        assert min(r["bins_used"]) >= 30  # the scene spans 0.05 .. 0.95
        errs.append(ref.sigma_error(r["alpha"], r["beta"], a0, b0))
    print(profile, "largest relative sigma error per seed:", ["%.4f" % e for e in errs])
    assert max(errs) <= BOUND, errs


def test_white_balance_gains():
    """The frame multiplied per colour after the clip and measured with those gains: the histogram of the unscaled frame
    where the float32 reciprocal round-trips (2 and 4 do), the accuracy bound where it does not (1.6)."""
    for profile in PROFILES:
        assert np.array_equal(smooth_hist(profile, 0, (2.0, 1.0, 4.0)), smooth_hist(profile, 0))
        a0, b0 = PROFILES[profile]
        errs = []
        for seed in SEEDS:
            r = ref.fit(smooth_hist(profile, seed, (2.0, 1.0, 1.6)), RGGB)
            errs.append(ref.sigma_error(r["alpha"], r["beta"], a0, b0))
        print(profile, "wb (2, 1, 1.6):", ["%.4f" % e for e in errs])
        assert max(errs) <= BOUND, errs
    g = ref.inv_gains(RGGB, (2.0, 1.0, 1.6))
    assert g.dtype == np.float32 and g[0] == np.float32(0.5) and g[1] == g[2] == 1 and g[3] == np.float32(1) / np.float32(1.6)
    assert np.array_equal(npf.inv_gains(RGGB, (2.0, 1.0, 1.6)), g) and np.array_equal(npf.inv_gains(None, None), np.ones(4))


def close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_library_fit_equals_the_numpy_fit():
    for profile in PROFILES:
        for seed in (0, 1, 2):
            for cfa in (RGGB, GRBG, None):
                for min_tiles in (16, 3):
                    h = smooth_hist(profile, seed)
                    want, got = ref.fit(h, cfa, min_tiles), npf.fit_profile(h, cfa, min_tiles)
                    assert got["bins_used"] == want["bins_used"]
                    assert close(got["alpha"], want["alpha"]) and close(got["beta"], want["beta"]), (got, want)
                    for (ga, gb), (wa, wb) in zip(got["per_colour"], want["per_colour"]):
                        assert close(ga, wa) and close(gb, wb)
                    if cfa is None:
                        assert got["per_colour"][0] == got["per_colour"][1] == got["per_colour"][2] == (got["alpha"], got["beta"])
    # a device-style int32 tensor on the host is taken as well
    t = torch.from_numpy(smooth_hist("high", 0).view(np.int32).copy())
    assert npf.fit_profile(t, RGGB) == npf.fit_profile(smooth_hist("high", 0), RGGB)


def hand_hist(points, planes=(0, 1, 2, 3)):
    """{mean bin: (energy bin, count)} in each of `planes`: the bin's median is the middle of the energy bin."""
    h = np.zeros((4, 64, 1024), np.uint32)
    for b, (k, n) in points.items():
        for p in planes:
            h[p, b, k] = n
    return h


def mid(k):
    lo = np.array([(k + ((127 - 32) << 5)) << 18], np.uint32).view(np.float32)[0]
    hi = np.array([(k + 1 + ((127 - 32) << 5)) << 18], np.uint32).view(np.float32)[0]
    return 0.5 * (float(lo) + float(hi))


def test_fit_by_hand():
    assert ref.edge(0) == 2.0 ** -32 and ref.edge(1024) == 1.0 and ref.edge(32) == 2.0 ** -31
    # two usable bins still fit: the line through the two points, whatever the weights
    (b1, k1), (b2, k2) = (8, 600), (40, 640)
    x1, x2, y1, y2 = (b1 + 0.5) / 64, (b2 + 0.5) / 64, mid(k1), mid(k2)
    alpha = (y2 - y1) / (x2 - x1)
    beta = y1 - alpha * x1
    assert alpha > 0 and beta > 0
    for fit in (ref.fit, npf.fit_profile):
        r = fit(hand_hist({b1: (k1, 20), b2: (k2, 50), 50: (700, 15)}), RGGB, 16)  # (bin 50: below min_tiles ... per plane)
        assert r["bins_used"] == [2, 3, 2]  # green adds two planes: 30 tiles in bin 50
        for c in (0, 2):
            assert abs(r["per_colour"][c][0] - alpha) <= 1e-9 * alpha and abs(r["per_colour"][c][1] - beta) <= 1e-9 * beta
    # an interpolated median: 10 tiles in bin k, 30 in bin k + 1 -> the 20th lies a third into bin k + 1
    h = hand_hist({b1: (k1, 20), b2: (k2, 10)})
    h[:, b2, k2 + 1] = 30
    want_y = ref.edge(k2 + 1) + (20 - 10) / 30 * (ref.edge(k2 + 2) - ref.edge(k2 + 1))
    for fit in (ref.fit, npf.fit_profile):
        a, b = fit(h, None, 16)["per_colour"][0]
        assert abs(a * x2 + b - want_y) <= 1e-9 * want_y
    # one usable bin: error -3 / ValueError naming the colour and its bin count
    one = hand_hist({b1: (k1, 20), b2: (k2, 50)}, planes=(1, 2))
    one[0, b1, k1] = one[3, b1, k1] = one[3, b2, k2] = 20  # RGGB: red has one bin, blue two
    ab, used = (ctypes.c_double * 8)(), (ctypes.c_int32 * 3)()
    lib = _lib.load()
    assert lib.hhsr_noise_profile_fit(one.ctypes.data_as(ctypes.c_void_p), _lib.cfa_bytes(RGGB), 16, ab, used) == -3
    assert list(used) == [1, 2, 2] and b"colour 0 has 1 usable" in lib.hhsr_last_error()
    with pytest.raises(ValueError, match="red has 1 usable mean bins"):
        npf.fit_profile(one, RGGB, 16)
    with pytest.raises(ValueError, match="red has 1 usable mean bins"):
        ref.fit(one, RGGB, 16)
    with pytest.raises(ValueError, match="0 usable mean bins"):
        npf.fit_profile(np.zeros((4, 64, 1024), np.uint32), None)
    assert lib.hhsr_noise_profile_fit(None, None, 16, ab, used) == -1 and b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_noise_profile_fit(one.ctypes.data_as(ctypes.c_void_p), None, 0, ab, used) == -1
    assert lib.hhsr_noise_profile_fit(one.ctypes.data_as(ctypes.c_void_p), _lib.cfa_bytes([[0, 3], [1, 2]]), 16, ab, used) == -1


def test_refits_by_hand():
    """Three points by hand: the free line has a negative intercept (then beta = 0, alpha = sum w x y / sum w x x) or a
    negative slope (then alpha = 0, beta = sum w y / sum w), weights n / y^2."""
    def sums(points):
        xs = [(b + 0.5) / 64 for b in points]
        ys = [mid(k) for k, _ in points.values()]
        ws = [4 * n / y ** 2 for (_, n), y in zip(points.values(), ys)]  # (four planes added: no CFA)
        return xs, ys, ws

    steep = {30: (400, 20), 40: (560, 30), 50: (600, 40)}  # y rises by orders of magnitude: intercept below 0
    xs, ys, ws = sums(steep)
    want = sum(w * x * y for w, x, y in zip(ws, xs, ys)) / sum(w * x * x for w, x in zip(ws, xs))
    for fit in (ref.fit, npf.fit_profile):
        r = fit(hand_hist(steep), None, 16)
        assert r["beta"] == 0.0 and abs(r["alpha"] - want) <= 1e-12 * want, r
    falling = {10: (640, 20), 30: (620, 30), 50: (600, 40)}
    xs, ys, ws = sums(falling)
    want = sum(w * y for w, y in zip(ws, ys)) / sum(ws)
    for fit in (ref.fit, npf.fit_profile):
        r = fit(hand_hist(falling), None, 16)
        assert r["alpha"] == 0.0 and abs(r["beta"] - want) <= 1e-12 * want, r


def test_restatement_bins():
    """The bin rule at its ends (a counted tile has e < 0.8: bin 1023 is the clamp for energies no tile can reach)."""
    e = np.array([2.0 ** -40, 2.0 ** -32, np.nextafter(np.float32(2.0 ** -31), 0), 2.0 ** -31, 0.5, 0.8, 1.0, 4.0], np.float32)
    b, k = ref.bins(np.array([0.0, 1 / 64, 0.999, 1.0, 0.5, 0.5, 0.5, 0.5]), e)
    assert list(k) == [0, 0, 31, 32, 992, 1011, 1023, 1023] and list(b) == [0, 1, 63, 63, 32, 32, 32, 32]


class Untouchable(dict):
    """A burst whose frames must not be looked at."""

    def __getitem__(self, k):
        raise AssertionError(f"burst[{k!r}] was read")

    get = __getitem__


@pytest.mark.parametrize("section,match", [({"source": "measure"}, "noise_model.source"),
                                           ({"source": "estimate", "alpha": 1e-4, "beta": 1e-6}, "contradicts"),
                                           ({"source": "estimate", "frames": 0}, "noise_model.frames"),
                                           ({"source": "estimate", "min_tiles": 2.5}, "noise_model.min_tiles")])
def test_bad_noise_options_are_refused_before_the_burst_is_read(section, match):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.noise_model.update(section)
    with pytest.raises(ValueError, match=match):
        hsr.process(Untouchable(), cfg)


def test_noise_options():
    from handheld_super_resolution.config import DEFAULTS

    cfg = hsr.default_config()
    assert npf.noise_options(cfg) == ("given", 1, 16) and "source" not in DEFAULTS["noise_model"]
    cfg.noise_model.update({"alpha": 1e-4, "beta": 1e-6, "source": "given"})
    assert npf.noise_options(cfg) == ("given", 1, 16)
    cfg.noise_model.update({"alpha": None, "beta": None, "source": "estimate", "frames": 3, "min_tiles": 8})
    assert npf.noise_options(cfg) == ("estimate", 3, 8)


def test_argument_refusals_do_not_touch_the_gpu():
    """Every refusal of include/hhsr.h returns -1 with "invalid argument" before any HIP call; every other argument is valid
    and the valid call, made first, does not return -1 (without a device it fails in the HIP runtime)."""
    lib = _lib.load()
    t = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    base = t.data_ptr() if t is not None else 1 << 32
    assert base % 256 == 0
    H, W = 32, 48
    frame_ptrs = [base + (1 << 21) + k * 16384 for k in range(_lib.MAX_BATCH + 1)]
    missed = []

    def table(ptrs):
        arr = (ctypes.c_void_p * len(ptrs))()
        for i, p in enumerate(ptrs):
            arr[i] = p
        return arr

    def call(**kw):
        a = dict(frames=None, n=3, H=H, W=W, rb=4 * W, cfa=_lib.cfa_bytes(RGGB), gains=_lib.floats([0.5, 1, 1, 0.625]),
                 hist=ctypes.c_void_p(base), off=0)
        a.update(kw)
        frames = table([p + a["off"] for p in frame_ptrs[:max(a["n"], 1)]]) if a["frames"] is None else a["frames"]
        return lib.hhsr_noise_profile_hist(frames, a["n"], a["H"], a["W"], a["rb"], a["cfa"], a["gains"], a["hist"], None)

    def refused(what, **kw):
        rc = call(**kw)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
            missed.append((what, rc, lib.hhsr_last_error()))

    assert call() >= 0 and call(cfa=None) >= 0 and call(n=1) >= 0 and call(n=_lib.MAX_BATCH) >= 0, lib.hhsr_last_error()
    assert call(rb=4 * W + 48) >= 0 and call(off=4) >= 0 and call(H=14, W=40, rb=160) >= 0, lib.hhsr_last_error()
    refused("null frames", frames=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    refused("a null frame", frames=table([frame_ptrs[0], 0, frame_ptrs[2]]))
    refused("null gains", gains=None)
    refused("null hist", hist=None)
    refused("hist off 4 bytes", hist=ctypes.c_void_p(base + 2))
    refused("n_frames 0", n=0)
    refused("n_frames above HHSR_MAX_BATCH", n=_lib.MAX_BATCH + 1)
    for k in ("H", "W"):
        refused(k + " odd", **{k: 33})
        refused(k + " = 0", **{k: 0})
        refused(k + " < 0", **{k: -2})
    refused("H beyond the grid", H=16 * 65536)
    refused("W beyond 32-bit row bytes", W=2 ** 30, rb=2 ** 40)
    refused("row_bytes below 4 W", rb=4 * W - 4)
    refused("row_bytes no multiple of 4", rb=4 * W + 2)
    refused("H row_bytes beyond int64", rb=2 ** 62)
    refused("frames off 4 bytes", off=2)
    refused("cfa entry above 2", cfa=_lib.cfa_bytes([[0, 1], [3, 2]]))
    if t is not None:
        torch.cuda.synchronize()
    assert not missed, missed


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
def ramp_frame(H, W, seed, cfa=None, wb=(1.0, 1.0, 1.0)):
    """Uniform noise around a ramp along x, its amplitude falling from 0.1 to 1e-4 down the frame: many mean and energy bins
    fill, and the tiles at the ramp's ends leave (0, 1)."""
    rng = np.random.default_rng(seed)
    amp = 10.0 ** (-1.0 - 3.0 * np.arange(H)[:, None] / H)
    f = (np.linspace(0.03, 0.97, W)[None, :] + amp * rng.uniform(-1, 1, (H, W))).astype(np.float32)
    return f if cfa is None else apply_wb(f, cfa, wb)


WB = (2.0, 1.0, 1.6)


@functools.lru_cache(maxsize=None)
def ramp_case(shape, cfa_name, seed=0):
    cfa = CFAS[cfa_name]
    f = ramp_frame(*shape, seed, cfa, WB)
    h = ref.histogram([f], cfa, WB)
    f.setflags(write=False)
    h.setflags(write=False)
    return f, h


def device_frame(frame, pad=0, offset=0):
    """The frame on the device with rows `pad` floats longer and its first value `offset` bytes behind a 256-byte
    boundary; everything around the pixels is NaN."""
    H, W = frame.shape
    stride = W + pad
    buf = torch.full((H * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0 and offset % 4 == 0
    view = buf[offset // 4: offset // 4 + H * stride].view(H, stride)[:, :W]
    view.copy_(torch.from_numpy(np.array(frame)))
    assert view.data_ptr() % 256 == offset and view.stride() == (stride, 1)
    return view


def gpu_hist(frames, cfa, wb=WB):
    return npf.noise_histogram(frames, cfa, wb).cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_histogram_equals_the_restatement(shape):
    H, W = shape
    for cfa_name, cfa in CFAS.items():
        f, want = ramp_case(shape, cfa_name)
        if H < 16:
            assert not want.any()
        elif (H, W) != (16, 16):
            assert np.count_nonzero(want) >= 4, "the case fills too few bins to tell anything"
        for pad in (0, 12):  # compact rows, and rows of 4 W + 48 bytes whose padding holds NaN
            for offset in (0, 16, 4):
                got = gpu_hist([device_frame(f, pad, offset)], cfa)
                assert np.array_equal(got, want), (shape, cfa_name, pad, offset, int(got.sum()), int(want.sum()))
    # three frames in one call = the sum of three single calls, in any order
    frames = [ramp_case(shape, "rggb", seed)[0] for seed in (0, 1, 2)]
    total = sum(ramp_case(shape, "rggb", seed)[1].astype(np.int64) for seed in (0, 1, 2)).astype(np.uint32)
    dev = [device_frame(f, 12, 0) for f in frames]
    assert np.array_equal(gpu_hist(dev, RGGB), total)
    assert np.array_equal(gpu_hist([dev[2], dev[0], dev[1]], RGGB), total)
    singles = sum(gpu_hist([d], RGGB).astype(np.int64) for d in dev)
    assert np.array_equal(singles, total.astype(np.int64))


@pytest.mark.gpu
def test_more_frames_than_a_batch():
    frames = [ramp_case((48, 80), "rggb", seed)[0] for seed in range(_lib.MAX_BATCH + 1)]
    total = sum(ramp_case((48, 80), "rggb", seed)[1].astype(np.int64) for seed in range(_lib.MAX_BATCH + 1))
    assert np.array_equal(gpu_hist([device_frame(f) for f in frames], RGGB).astype(np.int64), total)


def energy_bin(e):
    return int(min(1023, max(0, (int(np.array([e], np.float32).view(np.uint32)[0]) >> 18) - ((127 - 32) << 5))))


@pytest.mark.gpu
def test_tile_rules_by_hand():
    """One 32 x 32 monochrome frame, flat at 0.5: plane 0's tile (0, 0) is the pixels [0:16:2, 0:16:2].  One interior quad
    raised by d gives r = d there and -d / 4 at its four neighbours: S = 1.25 d^2, e = d^2 / 36, m = 0.5 + d / 64."""
    def run(edit):
        f = np.full((32, 32), 0.5, np.float32)
        tile = f[0:16:2, 0:16:2]
        edit(tile)
        h = gpu_hist([device_frame(f)], None, None)
        assert np.array_equal(h, ref.histogram([f], None)), "kernel != restatement"
        return h

    def only(h, b, k):
        want = np.zeros_like(h)
        want[0, b, k] = 1
        return np.array_equal(h, want)

    def bump(d):
        def edit(t):
            t[3, 3] = np.float32(0.5) + np.float32(d)
        return edit

    assert not run(lambda t: None).any()  # exactly flat tiles: e == 0
    d = 0.25
    assert only(run(bump(d)), int((0.5 + d / 64) * 64), energy_bin(np.float32(1.25 * d * d / 45.0)))
    assert int((0.5 + d / 64) * 64) == 32 and energy_bin(np.float32(1.25 * d * d / 45.0)) == 32 * (32 - 10) + 24  # 1.78 x 2^-10
    for bad in (0.0, 1.0, float("nan")):  # a clipped, a saturated, an undefined value: the tile does not count
        def edit(t, bad=bad):
            bump(d)(t)
            t[0, 7] = bad
        assert not run(edit).any(), bad
    d = 2.0 ** -14  # e = 2^-28 / 36 < 2^-32: bin 0
    assert np.float32(0.5) + np.float32(d) != np.float32(0.5) and 1.25 * d * d / 45.0 < 2.0 ** -32
    assert only(run(bump(d)), 32, 0)
    # the largest energy a counted tile can have: a checkerboard of eps and 1 - eps has |r| = 1 - 2 eps at the 36 interior
    # quads, e = 0.8 (1 - 2 eps)^2 < 0.8 — no tile reaches e >= 1, so bin 1023 is only the clamp of the rule; the top bin
    # that can fill is that of 0.8 = 1.6 x 2^-1: 32 * 31 + 19 = 1011
    eps = 2.0 ** -20

    def board(t):
        yy, xx = np.mgrid[0:8, 0:8]
        t[...] = np.where((yy + xx) % 2 == 0, np.float32(eps), np.float32(1 - eps))
    h = run(board)
    r = np.float32(1 - eps) - np.float32(0.25) * np.float32(4 * eps)
    e = np.float32(36 * float(r * r) / 45.0)
    assert only(h, 32, energy_bin(e)) and energy_bin(e) == 1011 and e < 0.8


@pytest.mark.gpu
def test_capture_and_replay():
    """Captured into a HIP graph and replayed twice the call gives the eager histogram, not twice that: it zeroes first."""
    f, want = ramp_case((48, 80), "rggb")
    d = device_frame(f, 12, 16)
    hist = torch.full(npf.HIST_SHAPE, 7, dtype=torch.int32, device="cuda")
    gains = _lib.floats(npf.inv_gains(RGGB, WB))
    cfa = _lib.cfa_bytes(RGGB)
    table = _lib.ptr_array([d])

    def launch():
        _lib.call("hhsr_noise_profile_hist", table, 1, 48, 80, d.stride(0) * 4, cfa, gains, _lib.ptr(hist), _lib.stream())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    hist.fill_(3)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want)


E2E_MIN_TILES = 4


def e2e_config(estimate=True):
    c = hsr.default_config()
    c.verbose = 0
    c.scale = 2
    c.block_matching.tuning.tile_size = 16
    c.block_matching.tuning.factors = [1, 2]
    c.block_matching.tuning.tile_size_factors = [1, 1]
    c.block_matching.tuning.search_radii = [1, 4]
    c.block_matching.tuning.metrics = ["L1", "L2"]
    c.noise_model.estimator = "analytic"  # (no Monte-Carlo run: the curves are not what is tested)
    if estimate:
        c.noise_model.source = "estimate"
        # one 256 x 384 frame has 384 tiles per plane for some 58 mean bins, about 7 a bin: with the default of 16 no red
        # bin is usable and process() raises the ValueError of fit_profile (checked below); 4 leaves 42 / 47 / 43 bins
        c.noise_model.min_tiles = E2E_MIN_TILES
    return c


@functools.lru_cache(maxsize=None)
def e2e_counts():
    """Three 256 x 384 frames of the smooth scene as 10-bit counts (black 64, white 1023), shifted by whole quads."""
    a, b = PROFILES["high"]
    scene = ref.smooth_scene(256 + 16, 384 + 16)
    out = []
    for n, (dy, dx) in enumerate(((0, 0), (2, 4), (6, 2))):
        f = ref.noisy(scene[dy:dy + 256, dx:dx + 384], a, b, 100 + n)
        out.append(np.clip(np.rint(f * (1023 - 64) + 64), 0, 1023).astype(np.uint16))
    return out


def e2e_burst(form):
    counts = e2e_counts()
    m = dict(cfa_pattern=RGGB, white_balance=[1.0, 1.0, 1.0])
    if form == "float32":  # the loader's float32 arithmetic (utils_dng.py:149-160) with unit gains
        fl = [(c.astype(np.float32) - np.float32(64)) / np.float32(1023 - 64) for c in counts]
        return dict(m, ref=fl[0], comp=np.stack(fl[1:])), fl[0]
    packed = [utils_dng.pack_raw(c, "mipi10") for c in counts]
    return dict(m, ref=packed[0], comp=np.stack(packed[1:]), packing="mipi10", black_levels=[64, 64, 64], white_level=1023), None


@pytest.mark.gpu
def test_process_estimates_the_profile():
    profiles = {}
    for form in ("float32", "mipi10"):
        burst, ref_float = e2e_burst(form)
        cfg = e2e_config()
        out, dbg = hsr.process(burst, cfg)
        assert out.shape == (512, 768, 3) and out.dtype == np.float32
        prof = dbg["noise profile"]
        assert sorted(prof) == ["alpha", "beta", "bins_used", "per_colour"]
        assert cfg.noise_model.alpha == prof["alpha"] and cfg.noise_model.beta == prof["beta"]
        profiles[form] = prof
        if ref_float is not None:
            assert prof == hsr.estimate_noise_profile(ref_float, RGGB, [1.0, 1.0, 1.0], E2E_MIN_TILES)
            assert prof == ref_fit_of(ref_float)  # and the library's fit of the kernel's histogram = the restatement's, closely
        with pytest.raises(ValueError, match="noise model \\(alpha, beta\\) missing"):
            hsr.process(burst, e2e_config(estimate=False))
    assert profiles["float32"] == profiles["mipi10"]
    # the estimate is a usable profile (256 x 384: the restatement's error at this size is below 10 %, PARITY.md; asserted
    # here only loosely, as a sanity check of the wiring — the accuracy test is the CPU one)
    a0, b0 = PROFILES["high"]
    assert ref.sigma_error(profiles["float32"]["alpha"], profiles["float32"]["beta"], a0, b0) < 0.25
    # frames: 3 measures the whole burst (clamped: 9 as well)
    burst, _ = e2e_burst("mipi10")
    cfg = e2e_config()
    cfg.noise_model.frames = 9
    _, dbg = hsr.process(burst, cfg)
    fl = [(c.astype(np.float32) - np.float32(64)) / np.float32(1023 - 64) for c in e2e_counts()]
    assert dbg["noise profile"] == hsr.estimate_noise_profile(np.stack(fl), RGGB, [1.0, 1.0, 1.0], E2E_MIN_TILES)
    # the default min_tiles on one frame of this size: the colour and its bin count are named
    cfg = e2e_config()
    cfg.noise_model.min_tiles = 16
    with pytest.raises(ValueError, match="red has 0 usable mean bins"):
        hsr.process(e2e_burst("float32")[0], cfg)
    assert dbg["noise profile"] != profiles["mipi10"]


def ref_fit_of(frame):
    """The library's fit of the restatement's histogram: equal to the profile of the kernel's histogram iff the histograms
    lead to the same fit (they are equal bit for bit: test_histogram_equals_the_restatement)."""
    return npf.fit_profile(ref.histogram([frame], RGGB, (1.0, 1.0, 1.0)), RGGB, E2E_MIN_TILES)
