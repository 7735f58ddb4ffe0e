"""White balance of a burst that brings none: without a GPU the NumPy restatement's accuracy against known gains, the gate
against a large coloured object, the library's host fit against the NumPy fit, the option checks and every refusal of
process() and of the C entry points; on the GPU hhsr_white_balance_hist against the restatement bit for bit (formats, CFAs,
strides, alignments, 16-bit content, tiles on both sides of every rule), the tile rules by hand, batches, contention, graph
capture, and process() with white_balance.source = estimate end to end."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import white_balance_ref as ref

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, synthetic as synth, utils_dng, white_balance as wbm

RGGB, BGGR, GRBG, GBRG = [[0, 1], [1, 2]], [[2, 1], [1, 0]], [[1, 0], [2, 1]], [[1, 2], [0, 1]]
CFAS = {"rggb": RGGB, "bggr": BGGR, "grbg": GRBG, "gbrg": GBRG}
GAINS = ((2.0, 1.0, 1.5), (1.3, 1.0, 2.6))
SEEDS = range(8)
BLACK10, WHITE10 = [64, 64, 64], 1023
# Largest relative error of the R and B gains on synthetic.make_burst(512, 768, 1, seed), seeds 0 .. 7, both gain triples,
# 10-bit counts with black level 64: measured with the restatement of this repository 1.17 % (seed 0 of both triples; the
# other seeds 0.1 - 0.8 %); asserted: twice the worst, because eight seeds bound the tail loosely (PARITY.md "White balance")
MEASURED_WORST = 0.0117
BOUND = 2 * MEASURED_WORST
# the kernel's tiling (csrc/hhsr_io.hip): a workgroup covers WB_SPAN_TILES = 32 tiles of 16 x 16 pixels side by side and
# WB_ROWS = 2 tile rows below each other
SPAN, ROWS = 32 * 16, 2 * 16
# the last two: two workgroups plus one tile along x = 32 x 1040, and one workgroup plus one tile row along y = 50 x 34
SHAPES = [(16, 16), (18, 34), (34, 50), (48, 80), (32, 2 * SPAN + 16), (ROWS + 18, 34)]
FORMATS = [("uint16", 16), ("mipi10", 10), ("mipi12", 12), ("mipi14", 14), ("be10", 10), ("be12", 12), ("be14", 14)]
BLACKS = (63.75, 64.0, 60.5)  # per colour; green's is an integer so that a green mean of exactly 1 / 64 exists


# ---- without a GPU ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed):
    s = synth.make_burst(512, 768, 1, seed)[0]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def scene_hist(seed, gains, block_rows=0):
    s = scene(seed) if not block_rows else ref.paint_block(scene(seed), RGGB, block_rows)
    h = ref.histogram([ref.camera(s, RGGB, gains, 64, WHITE10)], RGGB, BLACK10, WHITE10)
    h.setflags(write=False)
    return h


def test_restatement_accuracy_against_known_gains():
    errs = []
    for gains in GAINS:
        for seed in SEEDS:
            r = ref.fit(scene_hist(seed, gains))
            assert r["tiles"] >= 1300 and r["tiles_gated"] >= 0.95 * r["tiles"]  # of 1536: a few dark or clipped tiles
            errs.append(ref.gain_error(r["white_balance"], gains))
    print("largest relative gain error per (gains, seed):", ["%.4f" % e for e in errs])
    assert max(errs) <= BOUND, errs  # measured: 0.0117


def test_the_gate_throws_out_a_coloured_object():
    """A block of balanced colour (0.8, 0.15, 0.1) over the top 20 % and 35 % of the rows.  Gains (2, 1, 1.5): with
    (1.3, 1, 2.6) the block's m_G / m_R is below 1 / 4 and its tiles leave the histogram by the range rule, which would test
    nothing of the gate.  Measured: gated 0.45 % / 0.84 %, un-gated 29 % / 45 %."""
    gains = GAINS[0]
    for rows in (102, 179):
        h = scene_hist(0, gains, rows)
        gated, plain = ref.fit(h), ref.fit(h, gate=False)
        eg, ep = ref.gain_error(gated["white_balance"], gains), ref.gain_error(plain["white_balance"], gains)
        print(rows, "rows: gated %.4f, un-gated %.4f" % (eg, ep), gated["tiles"], gated["tiles_gated"])
        assert eg <= 0.05 and ep >= 0.20, (rows, eg, ep)
        assert gated["tiles_gated"] < 0.85 * gated["tiles"]
        lib = wbm.fit_white_balance(h)
        assert lib["tiles"] == gated["tiles"] and lib["tiles_gated"] == gated["tiles_gated"]
        assert close(lib["white_balance"][0], gated["white_balance"][0]) and close(lib["white_balance"][2], gated["white_balance"][2])


def close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def same_fit(got, want):
    return (got["tiles"] == want["tiles"] and got["tiles_gated"] == want["tiles_gated"] and got["white_balance"][1] == 1.0
            and close(got["white_balance"][0], want["white_balance"][0]) and close(got["white_balance"][2], want["white_balance"][2]))


def test_library_fit_equals_the_numpy_fit():
    for gains in GAINS:
        for seed in (0, 1, 2):
            for min_tiles in (16, 1):
                h = scene_hist(seed, gains)
                want, got = ref.fit(h, min_tiles), wbm.fit_white_balance(h, min_tiles)
                assert sorted(got) == ["tiles", "tiles_gated", "white_balance"] and same_fit(got, want), (got, want)
    # a device-style int32 tensor on the host is taken as well
    t = torch.from_numpy(scene_hist(0, GAINS[0]).view(np.int32).copy())
    assert wbm.fit_white_balance(t) == wbm.fit_white_balance(scene_hist(0, GAINS[0]))


def hand_hist(points):
    h = np.zeros((192, 192), np.uint32)
    for (u, v), n in points.items():
        h[u, v] = n
    return h


def test_fit_by_hand():
    assert close(ref.centre(64), np.log2(1 + 0.5 / 32)) and close(ref.centre(0), np.log2(0.25 * (1 + 0.5 / 32)))
    assert close(ref.centre(191), np.log2(8 * (1 + 31.5 / 32))) and close(ref.centre(128) - ref.centre(64), 2.0)
    for fit in (ref.fit, wbm.fit_white_balance):
        # a single bin: its centre
        r = fit(hand_hist({(100, 40): 64}), 16)
        assert r["tiles"] == r["tiles_gated"] == 64
        assert close(r["white_balance"][0], 2.0 ** ref.centre(100)) and close(r["white_balance"][2], 2.0 ** ref.centre(40))
        assert r["white_balance"][1] == 1.0
        # two clusters 2 octaves apart, 20 and 80 tiles: the centroid lies 0.4 octaves from the heavier one and 1.6 from
        # the lighter one, so the first gate holds the heavier one alone
        r = fit(hand_hist({(64, 64): 20, (128, 64): 80}), 16)
        assert r["tiles"] == 100 and r["tiles_gated"] == 80
        assert close(r["white_balance"][0], 2.0 ** ref.centre(128)) and close(r["white_balance"][2], 2.0 ** ref.centre(64))
        # two equal clusters: the centroid lies 1 octave from both, its gate is empty: it is kept, tiles_gated = 0
        r = fit(hand_hist({(64, 64): 50, (128, 64): 50}), 16)
        assert r["tiles"] == 100 and r["tiles_gated"] == 0
        assert close(r["white_balance"][0], 2.0 ** (0.5 * (ref.centre(64) + ref.centre(128))))
        assert close(r["white_balance"][2], 2.0 ** ref.centre(64))
        # the gate is a circle: a bin 0.49 octaves away in u AND in v (0.69 in all) is outside
        r = fit(hand_hist({(64, 64): 90, (77, 77): 10}), 16)
        assert r["tiles"] == 100 and r["tiles_gated"] == 90 and close(r["white_balance"][0], 2.0 ** ref.centre(64))
        # N = min_tiles - 1
        with pytest.raises(ValueError, match="15 usable tiles, fewer than min_tiles = 16"):
            fit(hand_hist({(64, 64): 15}), 16)
        assert fit(hand_hist({(64, 64): 16}), 16)["tiles"] == 16
    with pytest.raises(ValueError, match="white_balance.frames.*white_balance.min_tiles.*give the gains"):
        wbm.fit_white_balance(np.zeros((192, 192), np.uint32))
    with pytest.raises(ValueError, match="integer histogram"):
        wbm.fit_white_balance(np.zeros((4, 64, 1024), np.uint32))
    with pytest.raises(ValueError, match="min_tiles"):
        wbm.fit_white_balance(np.zeros((192, 192), np.uint32), 0)
    lib = _lib.load()
    wb, tiles = (ctypes.c_double * 3)(), (ctypes.c_int64 * 2)()
    few = hand_hist({(64, 64): 15})
    assert lib.hhsr_white_balance_fit(few.ctypes.data_as(ctypes.c_void_p), 16, wb, tiles) == -3
    assert list(tiles) == [15, 0] and list(wb) == [1.0, 1.0, 1.0] and b"15 usable tiles" in lib.hhsr_last_error()
    assert lib.hhsr_white_balance_fit(None, 16, wb, tiles) == -1 and b"invalid argument" in lib.hhsr_last_error()
    assert lib.hhsr_white_balance_fit(few.ctypes.data_as(ctypes.c_void_p), 0, wb, tiles) == -1


class Untouchable(dict):
    """A burst whose frames must not be looked at."""

    def __getitem__(self, k):
        raise AssertionError(f"burst[{k!r}] was read")

    get = __getitem__


def config_with(section, mode=None):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.white_balance = section
    if mode is not None:
        cfg.mode = mode
    return cfg


BAD_SECTIONS = [({"source": "measure"}, "white_balance.source"), ({"source": "auto"}, "white_balance.source"),
                ({"source": "estimate", "frames": 0}, "white_balance.frames"),
                ({"source": "estimate", "frames": 1.5}, "white_balance.frames"),
                ({"source": "estimate", "frames": True}, "white_balance.frames"),
                ({"source": "given", "frames": -1}, "white_balance.frames"),
                ({"source": "estimate", "min_tiles": 0}, "white_balance.min_tiles"),
                ({"source": "estimate", "min_tiles": "many"}, "white_balance.min_tiles")]


@pytest.mark.parametrize("section,match", BAD_SECTIONS)
def test_bad_options_are_refused_before_the_burst_is_read(section, match):
    with pytest.raises(ValueError, match=match):
        wbm.wb_options(config_with(section))
    with pytest.raises(ValueError, match=match):
        hsr.process(Untouchable(), config_with(section))


def test_wb_options():
    from handheld_super_resolution.config import DEFAULTS

    assert "white_balance" not in DEFAULTS
    assert wbm.wb_options(hsr.default_config()) == ("given", 1, 16)
    assert wbm.wb_options(config_with({"source": "given"})) == ("given", 1, 16)
    assert wbm.wb_options(config_with({"source": "estimate", "frames": 3, "min_tiles": 8})) == ("estimate", 3, 8)


def test_process_refuses_what_has_no_white_balance_to_estimate():
    """mode grey, a folder of .dng files, float frames and integer tensors: each a ValueError before anything is uploaded
    (without a GPU an upload would be a RuntimeError instead)."""
    est = {"source": "estimate"}
    with pytest.raises(ValueError, match="mode grey"):
        hsr.process(Untouchable(), config_with(est, mode="grey"))
    with pytest.raises(ValueError, match="folder of .dng"):
        hsr.process("some/folder/of/dngs", config_with(est))
    f = np.full((32, 48), 0.5, np.float32)
    meta = dict(cfa_pattern=RGGB, alpha=1e-4, beta=1e-6, black_levels=BLACK10, white_level=WHITE10)
    with pytest.raises(ValueError, match="needs integer sensor counts"):
        hsr.process(dict(meta, ref=f, comp=f[None]), config_with(est))
    t = torch.zeros((32, 48), dtype=torch.int32)
    with pytest.raises(ValueError, match="needs integer sensor counts"):
        hsr.process(dict(meta, ref=t, comp=t[None]), config_with(est))


def test_run_handheld_takes_the_override():
    import run_handheld

    args = run_handheld.parse_args(["--impath", "burst.npz", "--outpath", "out.png", "white_balance.source=estimate",
                                    "white_balance.frames=2"])
    assert wbm.wb_options(run_handheld.build_config(args)) == ("estimate", 2, 16)
    args = run_handheld.parse_args(["--impath", "burst.npz", "--outpath", "out.png"])
    assert wbm.wb_options(run_handheld.build_config(args)) == ("given", 1, 16)


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
        a = dict(frames=None, n=3, H=H, W=W, rb=2 * W, fmt=-1, cfa=_lib.cfa_bytes(RGGB), black=_lib.doubles(BLACKS),
                 white=1023.0, hist=ctypes.c_void_p(base), off=0)
        a.update(kw)
        frames = table([p + a["off"] for p in frame_ptrs[:max(a["n"], 1)]]) if a["frames"] is None else a["frames"]
        return lib.hhsr_white_balance_hist(frames, a["n"], a["H"], a["W"], a["rb"], a["fmt"], a["cfa"], a["black"],
                                           a["white"], a["hist"], None)

    def refused(what, **kw):
        rc = call(**kw)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
            missed.append((what, rc, lib.hhsr_last_error()))

    assert call() >= 0 and call(n=1) >= 0 and call(n=_lib.MAX_BATCH) >= 0, lib.hhsr_last_error()
    assert call(rb=2 * W + 6) >= 0 and call(off=2) >= 0 and call(H=14, W=40, rb=80) >= 0, lib.hhsr_last_error()
    assert call(fmt=1, rb=60) >= 0 and call(fmt=1, rb=61, off=1) >= 0 and call(fmt=6, rb=84) >= 0, lib.hhsr_last_error()
    refused("format 0 (float32)", fmt=0, rb=4 * W)
    refused("an unknown format", fmt=7)
    refused("a NULL cfa", cfa=None)
    refused("H odd", H=33)
    refused("W odd", W=47)
    refused("H = 0", H=0)
    refused("W < 0", W=-2)
    refused("row_bytes shorter than the row", rb=2 * W - 2)
    refused("packed row_bytes shorter than the row", fmt=1, rb=59)
    refused("uint16 row_bytes odd", rb=2 * W + 1)
    refused("H row_bytes beyond int64", rb=2 ** 62)
    refused("H beyond the grid", H=16 * 65536)
    refused("null frames", frames=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    refused("a null frame", frames=table([frame_ptrs[0], 0, frame_ptrs[2]]))
    refused("uint16 frames off 2 bytes", off=1)
    refused("null black levels", black=None)
    refused("null hist", hist=None)
    refused("hist off 4 bytes", hist=ctypes.c_void_p(base + 2))
    refused("n_frames 0", n=0)
    refused("n_frames above HHSR_MAX_BATCH", n=_lib.MAX_BATCH + 1)
    refused("cfa entry above 2", cfa=_lib.cfa_bytes([[0, 1], [3, 2]]))
    refused("cfa without a blue", cfa=_lib.cfa_bytes([[0, 1], [1, 1]]))
    refused("white level at a black level", white=64.0)
    if t is not None:
        torch.cuda.synchronize()
    assert not missed, missed


def test_python_refusals():
    with pytest.raises(ValueError, match="no frame"):
        wbm.white_balance_histogram([], RGGB, BLACK10, WHITE10)
    with pytest.raises(RuntimeError, match="on the GPU"):
        wbm.white_balance_histogram([torch.zeros((32, 48), dtype=torch.int16)], RGGB, BLACK10, WHITE10)
    with pytest.raises(TypeError, match="already white-balanced"):
        wbm.device_counts(np.zeros((32, 48), np.float32), "cpu")
    with pytest.raises(ValueError, match="outside the uint16 range"):
        wbm.device_counts(np.full((32, 48), 70000, np.int32), "cpu")
    assert wbm.device_counts(np.full((2, 2), 1023, np.int64), "cpu").dtype == torch.uint16


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
def white_of(bits):
    return float((1 << bits) - 1)


def level(c, m, bits):
    """The count of colour c whose normalised value is m."""
    return BLACKS[c] + m * (white_of(bits) - BLACKS[c])


def tile_pixels(cfa, ty, tx, colour):
    """(ys, xs) of the pixels of `colour` in tile (ty, tx), row-major."""
    ys, xs = np.mgrid[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
    sel = np.asarray(cfa)[ys & 1, xs & 1] == colour
    return ys[sel], xs[sel]


def set_sum(counts, cfa, ty, tx, colour, S):
    """The pixels of `colour` in tile (ty, tx) as equal as integers can be, adding up to S."""
    ys, xs = tile_pixels(cfa, ty, tx, colour)
    n = len(ys)
    counts[ys, xs] = S // n + (np.arange(n) < S % n)


def set_mean(counts, cfa, ty, tx, rgb, bits):
    for c in range(3):
        set_sum(counts, cfa, ty, tx, c, int(round((128 if c == 1 else 64) * level(c, rgb[c], bits))))


def edge_tiles(counts, cfa, bits):
    """20 tiles, row-major from tile 0, in pairs or runs that straddle one rule each -> {rule: [tile indices]}."""
    nbx = counts.shape[1] // 16
    sat = ref.sat_counts(BLACKS, white_of(bits))
    where = {}
    k = 0

    def tile():
        nonlocal k
        k += 1
        return divmod(k - 1, nbx)

    # a count equal to sat - 1, and one equal to sat (red)
    for name, value in (("below sat", sat[0] - 1), ("at sat", sat[0])):
        ty, tx = tile()
        set_mean(counts, cfa, ty, tx, (0.5, 0.5, 0.5), bits)
        ys, xs = tile_pixels(cfa, ty, tx, 0)
        counts[ys[5], xs[5]] = value
        where[name] = [k - 1]
    # a green mean of exactly 1 / 64: S / 128 - 64 = (white - 64) / 64, and one count less
    S = 8192 + 2 * int(white_of(bits) - 64)
    for name, s in (("mean 1/64", S), ("mean below 1/64", S - 1)):
        ty, tx = tile()
        set_mean(counts, cfa, ty, tx, (1.5 / 64, 1.0 / 64, 1.5 / 64), bits)
        set_sum(counts, cfa, ty, tx, 1, s)
        where[name] = [k - 1]
    # m_G / m_R around 1 / 4 (red sums one count apart) and m_G / m_B around 16 (blue sums one count apart)
    for name, colour, mg, ratio in (("q_r around 1/4", 0, 0.1, 0.25), ("q_b around 16", 2, 0.5, 16.0)):
        g = int(round(128 * level(1, mg, bits)))
        m_g = (g / 128 - BLACKS[1]) / (white_of(bits) - BLACKS[1])
        S0 = int(round(64 * level(colour, m_g / ratio, bits)))
        where[name] = []
        for d in range(-4, 4):
            ty, tx = tile()
            set_mean(counts, cfa, ty, tx, (0.2, mg, 0.2), bits)
            set_sum(counts, cfa, ty, tx, 1, g)
            set_sum(counts, cfa, ty, tx, colour, S0 + d)
            where[name].append(k - 1)
    return where


@functools.lru_cache(maxsize=None)
def case(shape, bits, cfa_name, seed=0):
    """(counts uint16 [H][W], histogram of the restatement, {rule: tiles}): random tiles whose chroma spans more than the
    histogram's range, dark and clipped ones among them, noise on every pixel; with 24 tiles or more the first 20 are
    edge_tiles.  Rows and columns behind the last whole tile hold the largest count."""
    H, W = shape
    cfa = CFAS[cfa_name]
    rng = np.random.default_rng(1000 * bits + 10 * seed + H + W)
    white = white_of(bits)
    counts = np.full((H, W), int(white), np.int64)
    nby, nbx = H // 16, W // 16
    for ty in range(nby):
        for tx in range(nbx):
            mg = 2.0 ** rng.uniform(-5.5, -0.2)
            m = (mg / 2.0 ** rng.uniform(-2.6, 4.6), mg, mg / 2.0 ** rng.uniform(-2.6, 4.6))
            if (ty, tx) == (0, 0):
                m = (0.25, 0.4, 0.3)
            for c in range(3):
                ys, xs = tile_pixels(cfa, ty, tx, c)
                v = level(c, min(m[c], 0.9), bits) * (1 + 0.05 * rng.uniform(-1, 1, len(ys)))
                counts[ys, xs] = np.clip(np.rint(v), 0, white)
            if (ty, tx) != (0, 0) and rng.uniform() < 0.1:
                counts[16 * ty + rng.integers(16), 16 * tx + rng.integers(16)] = white  # a clipped pixel
    where = edge_tiles(counts, cfa, bits) if nby * nbx >= 24 else {}
    counts = counts.astype(np.uint16)
    hist = ref.histogram([counts], cfa, BLACKS, white)
    counts.setflags(write=False)
    hist.setflags(write=False)
    return counts, hist, where


def test_the_cases_put_tiles_on_both_sides_of_every_rule():
    """(no GPU) what the bit-for-bit test relies on: the restatement keeps and drops the edge tiles as designed."""
    shape = SHAPES[4]
    for _, bits in FORMATS[:4]:
        for cfa_name, cfa in CFAS.items():
            counts, hist, where = case(shape, bits, cfa_name)
            keep = ref.tile_bins(counts, cfa, BLACKS, white_of(bits))[0].reshape(-1)
            assert keep[where["below sat"]].all() and not keep[where["at sat"]].any(), (bits, cfa_name)
            assert keep[where["mean 1/64"]].all() and not keep[where["mean below 1/64"]].any(), (bits, cfa_name)
            for name in ("q_r around 1/4", "q_b around 16"):
                k = keep[where[name]]
                assert k.any() and not k.all(), (bits, cfa_name, name, k)
            assert int(hist.sum()) == int(keep.sum()) and 30 <= keep.sum() <= keep.size - 20 and np.count_nonzero(hist) >= 20
            if bits == 16:
                assert counts.max() == 65535


def device_u16(counts, pad=0, offset=0):
    """The counts on the device as int16 bits with rows `pad` counts longer and the first count `offset` bytes behind a
    256-byte boundary; everything around the pixels is 0xFFFF."""
    H, W = counts.shape
    stride = W + pad
    buf = torch.full((H * stride + 64,), -1, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 256 == 0 and offset % 2 == 0
    view = buf[offset // 2: offset // 2 + H * stride].view(H, stride)[:, :W]
    view.copy_(torch.from_numpy(np.array(counts).view(np.int16)))
    assert view.data_ptr() % 256 == offset and view.stride() == (stride, 1)
    return view


def device_packed(counts, packing, pad=0, offset=0):
    """The counts packed on the device with rows `pad` bytes longer and the first byte `offset` bytes behind a 256-byte
    boundary; everything around the rows' own bytes is 0xFF."""
    H, W = counts.shape
    need = utils_dng.packed_row_bytes(W, packing)
    rb = need + pad
    rows = utils_dng.pack_raw(np.array(counts), packing, rb)
    rows[:, need:] = 0xFF
    buf = torch.full((H * rb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset: offset + H * rb].view(H, rb)
    view.copy_(torch.from_numpy(rows))
    assert view.data_ptr() % 256 == offset and view.stride() == (rb, 1)
    return view


def layouts(fmt, W):
    """(pad, offset) of the three layouts of a format: compact; rows padded to the next multiple of 16 bytes (packed: of 4)
    beyond their pixels; an odd number of padding counts (packed: an odd row_bytes) with the base off its alignment."""
    if fmt == "uint16":
        return [(0, 0), ((-W) % 8 + 8, 0), (3, 2)]
    need = utils_dng.packed_row_bytes(W, fmt)
    return [(0, 0), ((-need) % 4 + 4, 0), (2 if need % 2 else 1, 1)]


def gpu_hist(frames, cfa, bits, fmt, width):
    packing = None if fmt == "uint16" else fmt
    h = wbm.white_balance_histogram(frames, cfa, BLACKS, white_of(bits), packing, width if packing else None)
    assert h.shape == (192, 192) and h.dtype == torch.int32
    return h.cpu().numpy().view(np.uint32)


def device_frame(counts, fmt, pad=0, offset=0):
    return device_u16(counts, pad, offset) if fmt == "uint16" else device_packed(counts, fmt, pad, offset)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_histogram_equals_the_restatement(shape):
    H, W = shape
    for fmt, bits in FORMATS:
        for cfa_name, cfa in CFAS.items():
            counts, want, _ = case(shape, bits, cfa_name)
            assert want.sum() >= 1
            for pad, offset in layouts(fmt, W):
                got = gpu_hist([device_frame(counts, fmt, pad, offset)], cfa, bits, fmt, W)
                assert np.array_equal(got, want), (shape, fmt, cfa_name, pad, offset, int(got.sum()), int(want.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,bits", [FORMATS[0], FORMATS[1], FORMATS[5]], ids=lambda v: str(v))
def test_batches(fmt, bits):
    """Three frames in one call = the sum of three single calls, in any order; more than MAX_BATCH frames are chunked."""
    shape = (48, 80)
    n = _lib.MAX_BATCH + 1
    cases = [case(shape, bits, "grbg", seed) for seed in range(n)]
    dev = [device_frame(c[0], fmt, *layouts(fmt, 80)[2]) for c in cases]
    total3 = sum(c[1].astype(np.int64) for c in cases[:3])
    assert np.array_equal(gpu_hist(dev[:3], GRBG, bits, fmt, 80), total3)
    assert np.array_equal(gpu_hist([dev[2], dev[0], dev[1]], GRBG, bits, fmt, 80), total3)
    assert np.array_equal(sum(gpu_hist([d], GRBG, bits, fmt, 80).astype(np.int64) for d in dev[:3]), total3)
    assert len({c[1].tobytes() for c in cases}) == n  # (the frames differ)
    assert np.array_equal(gpu_hist(dev, GRBG, bits, fmt, 80), sum(c[1].astype(np.int64) for c in cases))


def bin_of(q):
    return int(np.array([q], np.float32).view(np.uint32)[0] >> 18) - ((127 - 2) << 5)


@pytest.mark.gpu
def test_tile_rules_by_hand():
    """A 32 x 48 frame of six constant tiles, black 0 and white 1024 (m = count / 1024 exactly, sat = 960): three are kept,
    with m_G / m_R and m_G / m_B = (1, 1), (2, 4), (0.75, 1); one holds a count of 960, one has a green of 15 / 1024 <
    1 / 64, one has m_G / m_R = 20."""
    assert bin_of(1.0) == 64 and bin_of(2.0) == 96 and bin_of(4.0) == 128 and bin_of(0.75) == 48
    assert bin_of(0.25) == 0 and bin_of(np.nextafter(np.float32(16), 0)) == 191 and bin_of(16.0) == 192
    tiles = [(512, 512, 512), (200, 400, 100), (400, 300, 300), (512, 512, 512), (15, 15, 15), (40, 800, 400)]
    f = np.zeros((32, 48), np.uint16)
    for k, rgb in enumerate(tiles):
        for c in range(3):
            ys, xs = tile_pixels(GBRG, k // 3, k % 3, c)
            f[ys, xs] = rgb[c]
    f[16 + 7, 9] = 960  # tile 3
    want = np.zeros((192, 192), np.uint32)
    want[64, 64] = want[96, 128] = want[48, 64] = 1
    assert np.array_equal(ref.histogram([f], GBRG, [0, 0, 0], 1024), want)

    def run(frame):
        h = wbm.white_balance_histogram([device_u16(frame)], GBRG, [0, 0, 0], 1024)
        return h.cpu().numpy().view(np.uint32)

    assert np.array_equal(run(f), want)
    f[16 + 7, 9] = 959  # one count below sat: tile 3 counts too
    want[64, 64] = 2
    assert np.array_equal(run(f), want)
    # pixels outside the whole tiles change nothing: (34, 50) against its (32, 48) corner
    for fmt, bits in FORMATS:
        big = case((34, 50), bits, "rggb")[0]
        corner = np.ascontiguousarray(big[:32, :48])
        a = gpu_hist([device_frame(big, fmt)], RGGB, bits, fmt, 50)
        b = gpu_hist([device_frame(corner, fmt)], RGGB, bits, fmt, 48)
        assert np.array_equal(a, b) and a.sum() >= 1, fmt


@pytest.mark.gpu
def test_frames_without_a_tile():
    for shape in ((14, 40), (40, 14)):
        f = np.full(shape, 500, np.uint16)
        for fmt, bits in (FORMATS[0], FORMATS[1]):
            assert not gpu_hist([device_frame(f, fmt)], RGGB, bits, fmt, shape[1]).any()
        with pytest.raises(ValueError, match="0 usable tiles, fewer than min_tiles = 16"):
            hsr.estimate_white_balance(f, RGGB, BLACK10, WHITE10)
        with pytest.raises(ValueError, match="0 usable tiles, fewer than min_tiles = 1 "):
            hsr.estimate_white_balance(utils_dng.pack_raw(f, "mipi10"), RGGB, BLACK10, WHITE10, packing="mipi10",
                                       width=shape[1], min_tiles=1)


@pytest.mark.gpu
def test_one_colour_everywhere():
    """512 x 768 of one colour: every tile adds to the same address — one bin holds 32 x 48 = 1536, every other bin 0."""
    f = np.tile(np.array([[300, 500], [500, 400]], np.uint16), (256, 384))
    want = ref.histogram([f], RGGB, BLACK10, WHITE10)
    assert want.max() == 1536 and np.count_nonzero(want) == 1
    for fmt in ("uint16", "mipi10"):
        d = device_frame(f, fmt)
        for n in (1, 3):  # (three times the same frame in one call: 4608)
            h = wbm.white_balance_histogram([d] * n, RGGB, BLACK10, WHITE10, None if fmt == "uint16" else fmt, 768)
            assert np.array_equal(h.cpu().numpy().view(np.uint32), n * want), (fmt, n)
    r = hsr.estimate_white_balance(f, RGGB, BLACK10, WHITE10)
    assert r["tiles"] == r["tiles_gated"] == 1536
    u, v = np.argwhere(want)[0]
    assert close(r["white_balance"][0], 2.0 ** ref.centre(u)) and close(r["white_balance"][2], 2.0 ** ref.centre(v))


@pytest.mark.gpu
def test_capture_and_replay():
    """Captured into a HIP graph and replayed twice the call gives the eager histogram, not twice that: it zeroes first."""
    counts, want, _ = case((48, 80), 10, "bggr")
    d = device_packed(counts, "mipi10", 1, 1)
    hist = torch.full(wbm.HIST_SHAPE, 7, dtype=torch.int32, device="cuda")
    cfa, black, table = _lib.cfa_bytes(BGGR), _lib.doubles(BLACKS), _lib.ptr_array([d])

    def launch():
        _lib.call("hhsr_white_balance_hist", table, 1, 48, 80, d.stride(0), utils_dng.PACKINGS["mipi10"], cfa, black,
                  white_of(10), _lib.ptr(hist), _lib.stream())

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


E2E_GAINS = (2.0, 1.0, 1.5)
E2E_MIN_TILES = 8   # one 128 x 192 frame has 96 tiles
E2E_NOISE_TILES = 2


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
        c.white_balance = {"source": "estimate", "min_tiles": E2E_MIN_TILES}
    return c


@functools.lru_cache(maxsize=None)
def e2e_counts():
    """Three 128 x 192 frames of the synthetic burst as the 10-bit counts of a sensor with the gains (2, 1, 1.5); frame 0 is
    smoothed along its rows (the mean with the next pixel of the same colour), so it is not the sharpest."""
    r, comp, _ = synth.make_burst(128, 192, 3, 7)
    out = [ref.camera(f, RGGB, E2E_GAINS, 64, WHITE10) for f in [r, *comp]]
    f0 = out[0].astype(np.int64)
    f0[:, :-2] = (f0[:, :-2] + f0[:, 2:]) // 2
    out[0] = f0.astype(np.uint16)
    return out


def e2e_burst(form, **extra):
    counts = e2e_counts()
    m = dict(cfa_pattern=RGGB, alpha=synth.ALPHA_ISO100, beta=synth.BETA_ISO100, black_levels=BLACK10, white_level=WHITE10)
    m.update(extra)
    if form == "uint16":
        return dict(m, ref=counts[0], comp=np.stack(counts[1:]))
    packed = [utils_dng.pack_raw(c, form) for c in counts]
    return dict(m, ref=packed[0], comp=np.stack(packed[1:]), packing=form)


@pytest.mark.gpu
def test_process_estimates_the_white_balance():
    results = {}
    for form in ("uint16", "mipi10"):
        cfg = e2e_config()
        out, dbg = hsr.process(e2e_burst(form), cfg)
        assert out.shape == (256, 384, 3) and out.dtype == np.float32
        wb = dbg["white balance"]
        assert sorted(wb) == ["tiles", "tiles_gated", "white_balance"] and wb["tiles"] <= 96
        assert list(cfg.exif.white_balance) == wb["white_balance"] and wb["white_balance"][1] == 1.0
        packing = None if form == "uint16" else form
        assert wb == hsr.estimate_white_balance(e2e_burst(form)["ref"], RGGB, BLACK10, WHITE10, packing, min_tiles=E2E_MIN_TILES)
        assert same_fit(wb, ref.estimate([e2e_counts()[0]], RGGB, BLACK10, WHITE10, E2E_MIN_TILES))
        # the image is that of the same burst with those gains given, and a given white_balance is ignored
        given, dbg2 = hsr.process(e2e_burst(form, white_balance=wb["white_balance"]), e2e_config(estimate=False))
        assert "white balance" not in dbg2 and np.array_equal(out, given, equal_nan=True)
        again, _ = hsr.process(e2e_burst(form, white_balance=[1.0, 1.0, 1.0]), e2e_config())
        assert np.array_equal(out, again, equal_nan=True)
        with pytest.raises(KeyError, match="white_balance"):
            hsr.process(e2e_burst(form), e2e_config(estimate=False))
        results[form] = (wb, out)
    assert results["uint16"][0] == results["mipi10"][0] and np.array_equal(results["uint16"][1], results["mipi10"][1], equal_nan=True)
    # a usable estimate (the crop's own channel means decide at this size: about 5 %; loosely, as a check of the wiring)
    assert ref.gain_error(results["uint16"][0]["white_balance"], E2E_GAINS) < 0.15
    # frames: 2 adds the next frame's counts; 9 is clamped to the burst's 3
    for frames, upto in ((2, 2), (9, 3)):
        cfg = e2e_config()
        cfg.white_balance.frames = frames
        _, dbg = hsr.process(e2e_burst("mipi10"), cfg)
        assert dbg["white balance"] == hsr.estimate_white_balance(np.stack(e2e_counts()[:upto]), RGGB, BLACK10, WHITE10,
                                                                  min_tiles=E2E_MIN_TILES)
        assert dbg["white balance"]["tiles"] > 96
    # too few tiles: the ValueError says what to do
    cfg = e2e_config()
    cfg.white_balance.min_tiles = 97
    with pytest.raises(ValueError, match="fewer than min_tiles = 97 .*white_balance.frames"):
        hsr.process(e2e_burst("uint16"), cfg)


@pytest.mark.gpu
def test_process_order_of_the_three_estimates():
    """reference.select = sharpest, white_balance.source = estimate and noise_model.source = estimate together: the gains come
    from the chosen frame's counts, the noise estimate uses the estimated gains — equal to the three steps done by hand."""
    counts = e2e_counts()
    for form in ("uint16", "mipi10"):
        cfg = e2e_config()
        cfg.reference = {"select": "sharpest", "candidates": 3}
        cfg.noise_model.source = "estimate"
        cfg.noise_model.min_tiles = E2E_NOISE_TILES
        out, dbg = hsr.process(e2e_burst(form), cfg)
        idx = dbg["reference index"]
        assert idx == int(np.argmax(dbg["sharpness"])) and idx != 0
        wb_hand = hsr.estimate_white_balance(counts[idx], RGGB, BLACK10, WHITE10, min_tiles=E2E_MIN_TILES)
        wb_first = hsr.estimate_white_balance(counts[0], RGGB, BLACK10, WHITE10, min_tiles=E2E_MIN_TILES)
        assert dbg["white balance"] == wb_hand and wb_hand != wb_first
        gains = wb_hand["white_balance"]
        ref_float = utils_dng.normalize_burst(counts[idx], BLACK10, WHITE10, gains, RGGB)
        noise_hand = hsr.estimate_noise_profile(ref_float, RGGB, gains, E2E_NOISE_TILES)
        assert dbg["noise profile"] == noise_hand
        assert noise_hand != hsr.estimate_noise_profile(ref_float, RGGB, [1.0, 1.0, 1.0], E2E_NOISE_TILES)
        assert list(cfg.exif.white_balance) == gains and cfg.noise_model.alpha == noise_hand["alpha"]
        # and the image is that of the reordered burst with both results given
        order = [idx] + [i for i in range(3) if i != idx]
        given = e2e_burst("uint16", white_balance=gains, alpha=noise_hand["alpha"], beta=noise_hand["beta"])
        given["ref"], given["comp"] = counts[order[0]], np.stack([counts[i] for i in order[1:]])
        want, _ = hsr.process(given, e2e_config(estimate=False))
        assert np.array_equal(out, want, equal_nan=True)
