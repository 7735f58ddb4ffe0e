"""Reference selection: the NumPy restatement of the sharpness score against hand-computed values, the argument checks
of hhsr_frame_sharpness and the selection rule without a GPU; on the GPU the kernel against the restatement, its
bitwise properties (stride, alignment, batch, position, format) and process() with config.reference end to end."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import sharpness_ref

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, utils_dng, utils_image, synthetic as synth
from handheld_super_resolution import super_resolution as sr

RGGB, BGGR, GRBG, GBRG = [[0, 1], [1, 2]], [[2, 1], [1, 0]], [[1, 0], [2, 1]], [[1, 2], [0, 1]]
LAYOUTS = ["mipi10", "mipi12", "mipi14", "be10", "be12", "be14"]
BITS = {"mipi10": 10, "mipi12": 12, "mipi14": 14, "be10": 10, "be12": 12, "be14": 14}

# the kernel's tiling (csrc/hhsr_io.hip: SHARP_TILE_QW x SHARP_TILE_QH quads): a workgroup covers 1008 x 64 pixels, a
# thread 16 pixels of two rows; a wave whose 16-pixel pieces are all whole and whose rows start on 16 bytes (packed: a
# dword) loads vectors, any other wave decides per piece and reads item by item
TILE_W, TILE_H = 1008, 64
BIG = (2 * TILE_H + 2, 2 * TILE_W + 2)  # two workgroups plus one quad along each axis
SHAPES = [(2, 2), (4, 4), (6, 10), (34, 70), BIG]  # (34, 70): W / 2 odd, a 6-pixel tail behind four whole pieces


# ---- without a GPU ------------------------------------------------------------------------------------------------------
FRAME44 = [[1, 2, 5, 7],
           [3, 4, 11, 13],
           [0, 8, 6, 2],
           [9, 1, 3, 10]]
# by hand.  greens at cell positions (1, 2): g = [[2.5, 9], [8.5, 2.5]] -> 6.5^2 + 6^2 + 6^2 + 6.5^2 = 156.5
#           greens at (0, 3): g = [[2.5, 9], [0.5, 8]] -> 6.5^2 + 7.5^2 + 2^2 + 1^2 = 103.5
#           no CFA: g = [[2.5, 9], [4.5, 5.25]] -> 6.5^2 + 0.75^2 + 2^2 + 3.75^2 = 60.875
#           greens at (0, 1): g = [[1.5, 6], [4, 4]] -> 4.5^2 + 0 + 2.5^2 + 2^2 = 30.5
HAND44 = [(RGGB, 156.5), (BGGR, 156.5), (GRBG, 103.5), (GBRG, 103.5), (None, 60.875), ([[1, 1], [0, 2]], 30.5)]


@pytest.mark.parametrize("cfa,want", HAND44, ids=["rggb", "bggr", "grbg", "gbrg", "mono", "gg.."])
def test_restatement_by_hand(cfa, want):
    for dtype in (np.float32, np.uint16, np.float64):
        f = np.array(FRAME44, dtype)
        assert sharpness_ref.score(f, cfa) == want
        t = sharpness_ref.terms(f, cfa)
        assert t.dtype == np.float32 and t.size == sharpness_ref.n_terms(4, 4) == 4
        assert sharpness_ref.score(f[:2, :2], cfa) == 0.0 and sharpness_ref.terms(f[:2, :2], cfa).size == 0
    f = np.array(FRAME44, np.float32)
    f[1, 2] = np.nan  # position 2 of quad (0, 1): green for RGGB / BGGR and without a CFA, not for the others
    s = sharpness_ref.score(f, cfa)
    assert math.isnan(s) == (cfa in (RGGB, BGGR, None)), (cfa, s)
    with pytest.raises(ValueError):
        sharpness_ref.score(np.zeros((3, 4), np.float32), cfa)
    with pytest.raises(ValueError):
        sharpness_ref.green_image(np.zeros((4, 4), np.float32), [[0, 1], [2, 2]])  # one green


def test_argument_refusals_do_not_touch_the_gpu():
    """Every refusal of include/hhsr.h returns -1 with "invalid argument" before any HIP call; every other argument of each
    call is valid, and the valid call is made first: it must not return -1 (without a device it fails in the HIP
    runtime).  hhsr_sharpness_workspace never shrinks when H, W or n_frames grow."""
    lib = _lib.load()
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    base = t.data_ptr() if t is not None else 1 << 32
    assert base % 256 == 0
    H, W = 6, 40
    frame_ptrs = [base + k * 4096 for k in range(_lib.MAX_BATCH + 1)]
    work, scores = ctypes.c_void_p(base + (1 << 19)), ctypes.c_void_p(base + (1 << 18))
    missed = []

    def table(ptrs):
        arr = (ctypes.c_void_p * len(ptrs))()
        for i, p in enumerate(ptrs):
            arr[i] = p
        return arr

    def row_bytes(fmt, w):
        if fmt > 0:
            out = ctypes.c_int64()
            assert lib.hhsr_packed_row_bytes(max(w, 1), min(fmt, 6), ctypes.byref(out)) == 0
            return out.value
        return (4 if fmt == 0 else 2) * w

    def call(**kw):
        a = dict(frames=None, n=3, H=H, W=W, rb=None, fmt=0, cfa=_lib.cfa_bytes(RGGB), work=work, wbytes=1 << 12,
                 scores=scores, off=0)
        a.update(kw)
        frames = table([p + a["off"] for p in frame_ptrs[:max(a["n"], 1)]]) if a["frames"] is None else a["frames"]
        rb = row_bytes(a["fmt"], a["W"]) if a["rb"] is None else a["rb"]
        return lib.hhsr_frame_sharpness(frames, a["n"], a["H"], a["W"], rb, a["fmt"], a["cfa"], a["work"], a["wbytes"],
                                        a["scores"], None)

    def refused(what, **kw):
        rc = call(**kw)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
            missed.append((what, rc, lib.hhsr_last_error()))

    for fmt in (0, -1, 1, 2, 3, 4, 5, 6):
        assert call(fmt=fmt) >= 0, (fmt, lib.hhsr_last_error())
        refused("row_bytes below the row's bytes", fmt=fmt, rb=row_bytes(fmt, W) - (4 if fmt == 0 else 2 if fmt < 0 else 1))
        assert call(fmt=fmt, rb=row_bytes(fmt, W) + 64) >= 0, (fmt, lib.hhsr_last_error())
    assert call(cfa=None) >= 0, lib.hhsr_last_error()  # no CFA: a monochrome sensor
    assert call(n=1) >= 0 and call(n=_lib.MAX_BATCH) >= 0, lib.hhsr_last_error()
    refused("null frames", frames=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))
    refused("a null frame", frames=table([frame_ptrs[0], 0, frame_ptrs[2]]))
    refused("null workspace", work=None)
    refused("null scores", scores=None)
    refused("n_frames 0", n=0)
    refused("n_frames < 0", n=-1)
    refused("n_frames above HHSR_MAX_BATCH", n=_lib.MAX_BATCH + 1)
    for k in ("H", "W"):
        refused(k + " odd", **{k: 7})
        refused(k + " = 0", **{k: 0})
        refused(k + " < 0", **{k: -2})
    refused("W beyond the 32-bit pixel indices", W=2**31 - 2, rb=2**40)
    refused("H beyond the grid", H=65535 * TILE_H + 2)
    refused("H row_bytes beyond int64", H=4096, rb=2**62)
    refused("one green", cfa=_lib.cfa_bytes([[0, 1], [2, 2]]))
    refused("three greens", cfa=_lib.cfa_bytes([[1, 1], [1, 2]]))
    refused("cfa entry above 2", cfa=_lib.cfa_bytes([[3, 1], [1, 2]]))
    refused("format 7", fmt=7, rb=4 * W)
    refused("format -2", fmt=-2, rb=4 * W)
    refused("float32 frames off 4 bytes", off=2)
    refused("uint16 frames off 2 bytes", fmt=-1, off=1)
    assert call(fmt=-1, off=2) >= 0 and call(fmt=0, off=4) >= 0 and call(fmt=1, off=1) >= 0, lib.hhsr_last_error()
    refused("float32 row_bytes no multiple of 4", rb=4 * W + 2)
    refused("workspace off 8 bytes", work=ctypes.c_void_p(base + (1 << 19) + 4))
    refused("scores off 8 bytes", scores=ctypes.c_void_p(base + (1 << 18) + 4))
    need = ctypes.c_size_t(5)
    assert lib.hhsr_sharpness_workspace(H, W, 3, ctypes.byref(need)) == 0 and need.value >= 3 * 8
    refused("workspace too small", wbytes=need.value - 1)
    assert call(wbytes=need.value) >= 0, lib.hhsr_last_error()

    def ws(h, w, n):
        out = ctypes.c_size_t()
        assert lib.hhsr_sharpness_workspace(h, w, n, ctypes.byref(out)) == 0, (h, w, n)
        return out.value

    sizes = [2, 4, 62, 64, 66, 130, 1024, 1026, 2050, 3000, 4000, 8192, 20000]
    for n in range(1, _lib.MAX_BATCH + 1):
        for a, b in zip(sizes, sizes[1:]):  # H W grows along each of these steps
            assert ws(a, a, n) <= ws(b, a, n) <= ws(b, b, n) and ws(a, a, n) <= ws(a, b, n) <= ws(b, b, n)
            assert n == 1 or ws(a, b, n - 1) < ws(a, b, n)
    assert ws(3000, 4000, 3) >= 8 * 2 * 256  # 12 MP x 3: at least two workgroups for each of the 256 CUs
    keep = ctypes.c_size_t(5)
    for h, w, n, out in ((0, 4, 1, keep), (4, 5, 1, keep), (4, 4, 0, keep), (4, 4, 9, keep), (4, 4, 1, None)):
        rc = lib.hhsr_sharpness_workspace(h, w, n, ctypes.byref(out) if out is not None else None)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error() and keep.value == 5):
            missed.append(("hhsr_sharpness_workspace", h, w, n, rc))
    if t is not None:
        torch.cuda.synchronize()
    assert not missed, missed


class Untouchable(dict):
    """A burst whose frames must not be looked at."""

    def __getitem__(self, k):
        raise AssertionError(f"burst[{k!r}] was read")

    get = __getitem__


@pytest.mark.parametrize("section", [{"select": "best"}, {"select": "sharpest", "candidates": 0},
                                     {"select": "first", "candidates": -1}, {"candidates": 2.5},
                                     {"select": "sharpest", "candidates": True}])
def test_bad_section_is_refused_before_the_burst_is_read(section):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.reference = section
    with pytest.raises(ValueError, match="config.reference"):
        hsr.process(Untouchable(), cfg)
    with pytest.raises(ValueError, match="config.reference"):
        sr.select_reference(None, [], cfg)


def test_selection_rule():
    nan, inf = float("nan"), float("inf")
    cases = [([1.0, 3.0, 2.0], 1), ([3.0, 3.0, 1.0], 0), ([1.0, 2.0, 2.0], 1), ([nan, 1.0, 0.5], 1), ([inf, 1.0, 2.0], 2),
             ([1.0, -inf, nan], 0), ([nan, nan, nan], 0), ([inf, nan, -inf], 0), ([nan, inf, 0.0], 2), ([0.0, 0.0], 0),
             ([5.0], 0), ([nan, nan, 0.0], 2)]
    for scores, want in cases:
        assert sr.pick_reference(scores) == want == sharpness_ref.select(scores), scores
        assert sr.pick_reference(np.array(scores)) == want
    cfg = hsr.default_config()
    assert sr.reference_options(cfg) == ("first", 3) and "reference" not in cfg
    assert sr.candidate_count(cfg, 20) == 3 and sr.candidate_count(cfg, 2) == 2 and sr.candidate_count(cfg, 1) == 1
    cfg.reference = {"select": "sharpest", "candidates": 50}
    assert sr.reference_options(cfg) == ("sharpest", 50)
    assert sr.candidate_count(cfg, 4) == 4  # more candidates than frames: the whole burst
    assert sharpness_ref.select([1.0, 2.0, 9.0], candidates=2) == 1 and sharpness_ref.select([1.0, 2.0], candidates=50) == 1
    # the section is no config.hip knob
    from handheld_super_resolution.config import HIP_KNOBS, DEFAULTS

    assert "reference" not in HIP_KNOBS and "reference" not in DEFAULTS
    ref, comp = np.zeros((2, 2), np.float32), np.arange(12, dtype=np.float32).reshape(3, 2, 2)
    r, c = sr.reorder_burst(ref, comp, 2)
    assert np.array_equal(r, comp[1]) and np.array_equal(c, np.stack([ref, comp[0], comp[2]]))
    lst = list(comp)
    r, c = sr.reorder_burst(ref, lst, 3)
    assert r is lst[2] and len(c) == 3 and c[0] is ref and c[1] is lst[0] and c[2] is lst[1]
    r, c = sr.reorder_burst(ref, comp, 0)
    assert r is ref and c is comp


# ---- on the GPU: the kernel against the restatement ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_of(shape):
    """(float32 frame in [0, 1), 10-bit counts as uint16) of a shape — made once, shared, never modified."""
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    f = rng.random(shape, dtype=np.float32)
    c = rng.integers(0, 1024, shape, dtype=np.uint16)
    f.setflags(write=False)
    c.setflags(write=False)
    return f, c


@functools.lru_cache(maxsize=None)
def want_of(shape, kind, cfa_key):
    cfa = None if cfa_key is None else [list(r) for r in cfa_key]
    return sharpness_ref.score(frames_of(shape)[0 if kind == "f32" else 1], cfa)


def key(cfa):
    return None if cfa is None else tuple(tuple(r) for r in cfa)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def scores(frames, cfa, **kw):
    return utils_image.frame_sharpness(frames, cfa, **kw).cpu().numpy()


def embed(frame, fill, row_items=None, lead=0, guard=64):
    """Device view [H, W] of `frame` inside a buffer filled with `fill`: `guard` items in front and behind, `lead` more
    items in front (the base pointer is then aligned to the item only), rows `row_items` apart."""
    H, W = frame.shape
    row_items = W if row_items is None else row_items
    buf = np.full(guard + lead + H * row_items + guard, fill, frame.dtype)
    buf[guard + lead: guard + lead + H * row_items].reshape(H, row_items)[:, :W] = frame
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev.as_strided((H, W), (row_items, 1), guard + lead)


def packed_ff(counts, name, row_bytes=None):
    """counts [H, W] -> uint8 [H, row_bytes] in which every bit that is no pixel's is 1 (padding pixels, trailing bits,
    row padding)."""
    H, W = counts.shape
    need = utils_dng.packed_row_bytes(W, name)
    ext = np.full((H, -(-W // 4) * 4), (1 << BITS[name]) - 1, np.uint16)
    ext[:, :W] = counts
    rows = utils_dng.pack_raw(ext, name)[:, :need]
    out = np.full((H, need if row_bytes is None else row_bytes), 0xFF, np.uint8)
    out[:, :need] = rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_restatement(shape):
    """|got - want| <= n_terms 2^-52 want, want = fsum of the float32 terms: the worst case of two float64 sums of
    non-negative terms in different orders."""
    H, W = shape
    n = sharpness_ref.n_terms(H, W)
    f, c = frames_of(shape)
    # (the four Bayer rotations, no CFA, and the four other placements of two greens: rows and columns)
    for cfa in (RGGB, BGGR, GRBG, GBRG, None, [[1, 1], [0, 2]], [[2, 0], [1, 1]], [[1, 0], [1, 2]], [[0, 1], [2, 1]]):
        for kind, frame in (("f32", f), ("u16", c)):
            want = want_of(shape, kind, key(cfa))
            dev = torch.from_numpy(frame.copy()).cuda()
            assert dev.data_ptr() % 256 == 0
            got = scores([dev], cfa)
            assert got.dtype == np.float64 and got.shape == (1,)
            print(f"{shape} {kind} cfa {cfa}: got {got[0]!r} want {want!r} bound {n * 2.0 ** -52 * want!r}")
            assert abs(got[0] - want) <= n * 2.0 ** -52 * want, (shape, kind, cfa, got[0], want)
            if shape == (2, 2):
                assert got[0] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 4), (34, 70), BIG], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_stride_alignment_batch_position(shape, kind):
    """The score of a frame — on its own, compact, 256-byte aligned — is the score of the same frame, bit for bit, with
    padded rows (padding and guard bands NaN / all-ones: not read), with a base pointer aligned to its item only, in calls
    of 1, 3 and MAX_BATCH frames at every position, beyond MAX_BATCH frames, and in a second call."""
    H, W = shape
    rng = np.random.default_rng(7)
    f0, c0 = frames_of(shape)
    src = f0 if kind == "f32" else c0
    fill = np.float32(np.nan) if kind == "f32" else np.uint16(0xFFFF)
    item = src.dtype.itemsize
    # MAX_BATCH + 3 different frames of the shape
    variants = [np.roll(src, k, axis=1).copy() if k else src.copy() for k in range(_lib.MAX_BATCH + 3)]
    for k, v in enumerate(variants[1:], 1):
        v[(k * 3) % H, (k * 5) % W] = src.max()
    compact = [torch.from_numpy(v).cuda() for v in variants]
    assert all(t.data_ptr() % 256 == 0 for t in compact)
    for cfa in (RGGB, GRBG, None):
        alone = np.concatenate([scores([t], cfa) for t in compact])
        assert np.isfinite(alone).all() and (len(set(alone.tolist())) > 1 or shape == (2, 2))
        assert np.array_equal(bits(alone), bits(np.concatenate([scores([t], cfa) for t in compact])))  # a second call
        for n in (1, 3, _lib.MAX_BATCH, _lib.MAX_BATCH + 3):
            for order in (list(range(n)), list(range(n))[::-1], list(rng.permutation(n))):
                got = scores([compact[i] for i in order], cfa)
                assert np.array_equal(bits(got), bits(alone[order])), (shape, kind, cfa, n, order)
        for row_items in (W + 1, W + 16 // item, W + 16 // item + 3):
            for lead in (0, 1):
                views = [embed(v, fill, row_items, lead) for v in variants[:3]]
                assert all(t.data_ptr() % 16 == (lead * item) % 16 for t in views)
                got = scores(views, cfa)
                assert np.array_equal(bits(got), bits(alone[:3])), (shape, kind, cfa, row_items, lead)
        views = [embed(v, fill, None, 1) for v in variants[:3]]  # compact rows, base on the item only
        assert np.array_equal(bits(scores(views, cfa)), bits(alone[:3])), (shape, kind, cfa, "item-aligned base")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 10), (34, 70), BIG], ids=lambda s: "x".join(map(str, s)))
def test_formats_agree(shape):
    """uint16 counts, the float32 frame holding the same counts and each of the six packed layouts of those counts score
    the same bits — packed rows compact, and padded with 0xFF bytes from an odd base."""
    H, W = shape
    counts = frames_of(shape)[1]
    for cfa in (RGGB, GBRG, None):
        want = scores([torch.from_numpy(counts.copy()).cuda()], cfa)
        assert np.isfinite(want).all() and want[0] > 0
        assert np.array_equal(bits(scores([torch.from_numpy(counts.astype(np.float32)).cuda()], cfa)), bits(want))
        for name in LAYOUTS:
            need = utils_dng.packed_row_bytes(W, name)
            rows = packed_ff(counts, name)
            got = scores([torch.from_numpy(rows).cuda()], cfa, packing=name, width=W)
            assert np.array_equal(bits(got), bits(want)), (shape, cfa, name, "compact")
            for rb, lead in ((need + 3, 1), (-(-need // 4) * 4 + 4, 0)):
                wide = packed_ff(counts, name, rb)
                view = embed(wide, np.uint8(0xFF), None, lead).as_strided((H, need), (rb, 1), 64 + lead)
                got = scores([view, view], cfa, packing=utils_dng.PACKINGS[name], width=W)
                assert np.array_equal(bits(got), bits(np.repeat(want, 2))), (shape, cfa, name, rb, lead)
    with pytest.raises(TypeError):
        scores([torch.zeros(4, 4, dtype=torch.float64, device="cuda")], RGGB)
    with pytest.raises(ValueError):
        scores([torch.zeros(4, 4, device="cuda"), torch.zeros(4, 6, device="cuda")], RGGB)
    with pytest.raises(RuntimeError, match="invalid argument"):
        scores([torch.zeros(4, 5, device="cuda")], RGGB)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 4), (34, 70), BIG], ids=lambda s: "x".join(map(str, s)))
def test_nan_stays_in_its_frame(shape):
    H, W = shape
    f = frames_of(shape)[0]
    for cfa, (y, x) in ((RGGB, (H - 1, W - 2)), (GRBG, (0, 0)), (None, (H // 2, W // 2))):
        bad = f.copy()
        bad[y, x] = np.nan  # a green position of its quad
        devs = [torch.from_numpy(a.copy()).cuda() for a in (f, bad, f[::-1], bad, f)]
        got = scores(devs, cfa)
        alone = scores([devs[0]], cfa)
        assert np.isnan(got[1]) and np.isnan(got[3]) and np.isfinite(got[[0, 2, 4]]).all(), (shape, cfa, got)
        assert bits(got[0]) == bits(alone[0]) == bits(got[4]), (shape, cfa)
        inf = f.copy()
        inf[y, x] = np.inf
        assert not np.isfinite(scores([torch.from_numpy(inf).cuda()], cfa)[0])  # Inf propagates (Inf, or NaN from Inf - Inf)


# ---- on the GPU: process() ------------------------------------------------------------------------------------------------
SHARP = 2  # the one frame of the burst that is not blurred


def blur121(frame):
    """Separable 1-2-1 blur of each of the four CFA planes (edge replicated)."""
    out = np.empty_like(frame)
    for i in range(2):
        for j in range(2):
            p = np.pad(frame[i::2, j::2].astype(np.float32), 1, mode="edge")
            p = (p[:-2] + 2 * p[1:-1] + p[2:]) * np.float32(0.25)
            out[i::2, j::2] = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]) * np.float32(0.25)
    return out


@functools.lru_cache(maxsize=None)
def blurred_burst():
    ref, comp, _ = synth.make_burst(64, 96, 4, seed=4)
    frames = [ref] + list(comp)
    frames = [f.copy() if k == SHARP else blur121(f) for k, f in enumerate(frames)]
    s = [sharpness_ref.score(f, RGGB) for f in frames]
    blurred = [v for k, v in enumerate(s) if k != SHARP]
    print("NumPy scores", s, "ratio", max(blurred) / s[SHARP])
    assert max(blurred) <= 0.2 * s[SHARP], s  # precondition: rounding cannot flip the choice
    for f in frames:
        f.setflags(write=False)
    return frames


def burst_config(section="absent"):
    c = hsr.default_config()
    c.verbose = 0
    c.scale = 2
    c.block_matching.tuning.tile_size = 16
    c.block_matching.tuning.factors = [1, 2]
    c.block_matching.tuning.tile_size_factors = [1, 1]
    c.block_matching.tuning.search_radii = [1, 4]
    c.block_matching.tuning.metrics = ["L1", "L2"]
    if section != "absent":
        c.reference = section
    return c


def burst_of(frames, form):
    """The burst mapping of a list of float frames in one of the three input forms (noise curves given: no Monte-Carlo)."""
    std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    m = dict(cfa_pattern=RGGB, white_balance=[1.0, 1.0, 1.0], alpha=synth.ALPHA_ISO100, beta=synth.BETA_ISO100,
             std_curve=std, diff_curve=diff)
    if form == "float32":
        return dict(m, ref=frames[0].copy(), comp=np.stack(frames[1:]))
    counts = [np.clip(np.rint(f * (1023 - 64) + 64), 0, 1023).astype(np.uint16) for f in frames]
    m.update(black_levels=[64, 64, 64], white_level=1023)
    if form == "uint16":
        return dict(m, ref=counts[0], comp=np.stack(counts[1:]))
    packed = [utils_dng.pack_raw(c, "mipi10") for c in counts]
    return dict(m, ref=packed[0], comp=np.stack(packed[1:]), packing="mipi10")


def candidates_of(frames, form):
    """What the score sees of each frame in a form: the float values, or the counts."""
    if form == "float32":
        return frames
    return [np.clip(np.rint(f * (1023 - 64) + 64), 0, 1023).astype(np.uint16) for f in frames]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["float32", "uint16", "mipi10"])
def test_process_picks_the_sharp_frame(form):
    """process() with select: sharpest reports frame 2 and returns the bits of process() on the burst reordered by hand
    with the section absent; the reported scores are the kernel's, within the bound of the restatement."""
    frames = blurred_burst()
    np_scores = [sharpness_ref.score(f, RGGB) for f in candidates_of(frames, form)]
    assert max(np_scores[:2] + np_scores[3:]) <= 0.2 * np_scores[SHARP], np_scores
    got, dbg = hsr.process(burst_of(frames, form), burst_config({"select": "sharpest", "candidates": 3}))
    assert dbg["reference index"] == SHARP
    s = dbg["sharpness"]
    assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (3,)
    n = sharpness_ref.n_terms(64, 96)
    assert all(abs(s[k] - np_scores[k]) <= n * 2.0 ** -52 * np_scores[k] for k in range(3)), (s, np_scores)
    by_hand = [frames[2], frames[0], frames[1], frames[3]]
    want, wdbg = hsr.process(burst_of(by_hand, form), burst_config())
    assert "reference index" not in wdbg and "sharpness" not in wdbg
    assert same_bits(got, want), form
    plain, _ = hsr.process(burst_of(frames, form), burst_config())
    assert not same_bits(plain, want)  # the choice matters: the blurred frame 0 as the base gives another image


@pytest.mark.gpu
def test_process_candidates_and_first():
    frames = blurred_burst()
    np_scores = [sharpness_ref.score(f, RGGB) for f in frames]
    pick = sharpness_ref.select(np_scores, candidates=2)
    assert abs(np_scores[0] - np_scores[1]) > 1e-6 * max(np_scores[:2])  # no tie that rounding could flip
    got, dbg = hsr.process(burst_of(frames, "float32"), burst_config({"select": "sharpest", "candidates": 2}))
    assert dbg["reference index"] == pick and dbg["sharpness"].shape == (2,)
    order = [pick] + [k for k in range(4) if k != pick]
    want, _ = hsr.process(burst_of([frames[k] for k in order], "float32"), burst_config())
    assert same_bits(got, want)
    absent, adbg = hsr.process(burst_of(frames, "float32"), burst_config())
    for section in ({"select": "first"}, {"select": "first", "candidates": 3}, {}):
        got, dbg = hsr.process(burst_of(frames, "float32"), burst_config(section))
        assert same_bits(got, absent) and sorted(dbg) == sorted(adbg), section
    # more candidates than frames: the whole burst is scored
    got, dbg = hsr.process(burst_of(frames, "float32"), burst_config({"select": "sharpest", "candidates": 9}))
    assert dbg["reference index"] == SHARP and dbg["sharpness"].shape == (4,)
    # select_reference on device tensors, and on a monochrome burst (no CFA: the mean of each quad)
    cfg = burst_config({"select": "sharpest"})
    idx, s = sr.select_reference(torch.from_numpy(frames[0].copy()).cuda(),
                                 [torch.from_numpy(f.copy()).cuda() for f in frames[1:]], cfg, cfa_pattern=RGGB)
    assert idx == SHARP and s.shape == (3,)
    cfg.mode = "grey"
    idx, s = sr.select_reference(frames[0], np.stack(frames[1:]), cfg)
    mono = [sharpness_ref.score(f, None) for f in frames[:3]]
    assert idx == sharpness_ref.select(mono)
    assert all(abs(a - b) <= sharpness_ref.n_terms(64, 96) * 2.0 ** -52 * b for a, b in zip(s, mono))
