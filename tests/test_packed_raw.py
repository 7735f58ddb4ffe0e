"""Packed 10/12/14-bit raw frames: the NumPy packers of utils_dng against known bytes, the argument checks of
hhsr_normalize_raw_packed without a GPU, and on the GPU the kernel, main() and process() bit for bit against the
uint16 path (which the oracle pins)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from helpers import assert_close

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, utils_dng, synthetic as synth

LAYOUTS = ["mipi10", "mipi12", "mipi14", "be10", "be12", "be14"]
BITS = {"mipi10": 10, "mipi12": 12, "mipi14": 14, "be10": 10, "be12": 12, "be14": 14}
# the pixels 3FF 000 155 2AA 001 (10 bits), FFF 000 555 AAA 001 (12), 3FFF 0000 1555 2AAA 0001 (14), packed by hand
PIXELS = {10: [0x3FF, 0x000, 0x155, 0x2AA, 0x001], 12: [0xFFF, 0x000, 0x555, 0xAAA, 0x001],
          14: [0x3FFF, 0x0000, 0x1555, 0x2AAA, 0x0001]}
KNOWN = {"mipi10": "FF 00 55 AA 93 00 00 00 00 01", "be10": "FF C0 05 56 AA 00 40",
         "mipi12": "FF 00 0F 55 AA A5 00 00 01", "be12": "FF F0 00 55 5A AA 00 10",
         "mipi14": "FF 00 55 AA 3F 50 A9 00 00 00 00 01 00 00", "be14": "FF FC 00 05 55 6A AA 00 04"}
CFA, BL, WB = [[2, 1], [1, 0]], [63, 64, 66], [1.91, 1.0, 1.57]


def table_row_bytes(W, name):
    """The issue's table, written out independently of the library."""
    B = BITS[name]
    if name.startswith("be"):
        return -(-W * B // 8)
    return {10: 5 * -(-W // 4), 12: 3 * -(-W // 2), 14: 7 * -(-W // 4)}[B]


def pack_ff(counts, name, row_bytes=None, frame_bytes=None, base=0):
    """counts [n, H, W] -> flat uint8 buffer in which everything that is not a pixel's bit is 1: the padding pixels of the
    last group and the trailing bits of a row (the counts are extended with all-ones pixels before they are packed), the
    row padding, the bytes between frames and the `base` bytes in front.  Returns (buffer, row_bytes, frame_bytes)."""
    n, H, W = counts.shape
    need = table_row_bytes(W, name)
    ext = np.full((n, H, -(-W // 4) * 4), (1 << BITS[name]) - 1, np.uint16)
    ext[..., :W] = counts
    rows = utils_dng.pack_raw(ext, name)[..., :need]
    rb = need if row_bytes is None else row_bytes
    fb = H * rb if frame_bytes is None else frame_bytes
    buf = np.full(base + (n - 1) * fb + H * rb, 0xFF, np.uint8)
    for k in range(n):
        frame = buf[base + k * fb: base + k * fb + H * rb].reshape(H, rb)
        frame[:, :need] = rows[k]
    return buf, rb, fb


# ---- without a GPU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts(name):
    B = BITS[name]
    assert utils_dng.PACKINGS == {n: i + 1 for i, n in enumerate(["mipi10", "mipi12", "mipi14", "be10", "be12", "be14"])}
    known = np.array([int(v, 16) for v in KNOWN[name].split()], np.uint8)
    px = np.array(PIXELS[B], np.uint16)
    got = utils_dng.pack_raw(px, name)
    assert got.dtype == np.uint8 and np.array_equal(got, known), (name, got.tolist())
    assert np.array_equal(utils_dng.unpack_raw(known, 5, name), px)
    rng = np.random.default_rng(B)
    for W in range(1, 71):
        need = table_row_bytes(W, name)
        assert utils_dng.packed_row_bytes(W, name) == need == utils_dng.packed_row_bytes(W, utils_dng.PACKINGS[name])
        p = rng.integers(0, 1 << B, (2, 3, W), dtype=np.uint16)
        packed = utils_dng.pack_raw(p, name)
        assert packed.shape == (2, 3, need)
        back = utils_dng.unpack_raw(packed, W, name)
        assert back.dtype == np.uint16 and np.array_equal(back, p), (name, W)
        wide = utils_dng.pack_raw(p, name, row_bytes=need + 5)  # a larger row_bytes is honoured: same bytes, zero padding
        assert wide.shape == (2, 3, need + 5) and np.array_equal(wide[..., :need], packed) and not wide[..., need:].any()
        # everything that is not a pixel's bit set to 1: group padding, trailing bits, row padding
        buf, rb, _ = pack_ff(p, name, row_bytes=need + 5)
        ff = buf.reshape(2, 3, rb)
        assert (ff[..., need:] == 0xFF).all() and np.array_equal(utils_dng.unpack_raw(ff, W, name), p), (name, W)
    with pytest.raises(ValueError):
        utils_dng.pack_raw(px, name, row_bytes=table_row_bytes(5, name) - 1)
    with pytest.raises(ValueError):
        utils_dng.pack_raw(np.array([1 << B]), name)
    with pytest.raises(ValueError):
        utils_dng.packed_row_bytes(8, "mipi8")
    with pytest.raises(RuntimeError, match="invalid argument"):
        utils_dng.packed_row_bytes(0, name)


def test_argument_refusals_do_not_touch_the_gpu():
    """Every refusal of include/hhsr.h returns -1 with "invalid argument" before any HIP call.  Every other argument of
    each call is valid and the valid call itself is made first: it must not return -1 (it launches on a device and fails
    in the HIP runtime without one).  Without a device nothing can launch, so arbitrary aligned addresses do."""
    lib = _lib.load()
    t = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    base = t.data_ptr() if t is not None else 1 << 32
    assert base % 256 == 0
    raw, out = ctypes.c_void_p(base), ctypes.c_void_p(base + (1 << 19))
    n, H, W = 2, 4, 37
    cfa, bl, wb = _lib.cfa_bytes(CFA), _lib.doubles(BL), _lib.doubles(WB)
    missed = []

    def call(**kw):
        a = dict(raw=raw, n=n, H=H, W=W, rb=None, fb=None, packing=1, cfa=cfa, bl=bl, wl=1023.0, wb=wb, out=out)
        a.update(kw)
        need = table_row_bytes(max(a["W"], 1), LAYOUTS[min(max(a["packing"], 1), 6) - 1])
        rb = need if a["rb"] is None else a["rb"]
        fb = a["H"] * rb if a["fb"] is None else a["fb"]
        return lib.hhsr_normalize_raw_packed(a["raw"], a["n"], a["H"], a["W"], rb, fb, a["packing"], a["cfa"], a["bl"],
                                             a["wl"], a["wb"], a["out"], None)

    def refused(what, **kw):
        rc = call(**kw)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
            missed.append((what, rc, lib.hhsr_last_error()))

    for packing in range(1, 7):
        need = table_row_bytes(W, LAYOUTS[packing - 1])
        assert call(packing=packing) >= 0, lib.hhsr_last_error()
        refused("row_bytes below the table", packing=packing, rb=need - 1)
        refused("frame_bytes < H row_bytes", packing=packing, rb=need + 3, fb=H * (need + 3) - 1)
        assert call(packing=packing, n=1, fb=0) >= 0, lib.hhsr_last_error()  # one frame: frame_bytes is not read
    for k in ("raw", "cfa", "bl", "wb", "out"):
        refused("null " + k, **{k: None})
    refused("packing 0", packing=0)
    refused("packing 7", packing=7)
    for k in ("W", "H", "n"):
        refused(k + " = 0", **{k: 0})
        refused(k + " < 0", **{k: -1})
    refused("n_frames above the grid limit", n=65536)
    refused("H above the grid limit", H=65536)
    refused("W above the 32-bit pixel indices of a row's last workgroup", W=2**31 - 1 - 4095)
    refused("cfa[k] > 2", cfa=_lib.cfa_bytes([[0, 1], [1, 3]]))
    refused("white == black", wl=66.0)
    refused("wb[1] == 0", wb=_lib.doubles([1.9, 0.0, 1.6]))
    refused("misaligned out", out=ctypes.c_void_p(base + (1 << 19) + 4))
    assert call(raw=ctypes.c_void_p(base + 1), rb=table_row_bytes(W, "mipi10") + 3) >= 0  # raw needs no alignment
    got = ctypes.c_int64(-5)
    for W_, packing in ((0, 1), (-3, 4), (16, 0), (16, 7)):
        rc = lib.hhsr_packed_row_bytes(W_, packing, ctypes.byref(got))
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error() and got.value == -5):
            missed.append(("hhsr_packed_row_bytes", W_, packing, rc))
    if not (lib.hhsr_packed_row_bytes(16, 1, None) == -1 and b"invalid argument" in lib.hhsr_last_error()):
        missed.append(("hhsr_packed_row_bytes", "null"))
    assert lib.hhsr_packed_row_bytes(2**31 - 1, 6, ctypes.byref(got)) == 0 and got.value == -(-(2**31 - 1) * 14 // 8)
    if t is not None:
        torch.cuda.synchronize()
    assert not missed, missed


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 6, 70), (2, 5, 64), (1, 2, 3), (2, 4, 4117)]  # 4117: two workgroups (4096 pixels each) and a 5-pixel tail


@functools.lru_cache(maxsize=None)
def counts_and_reference(B, shape):
    """{pattern: (counts, oracle result)} — computed once per (bits, shape), shared by the layouts, never modified."""
    n, H, W = shape
    rng = np.random.default_rng(B * 1000 + W)
    walk = np.broadcast_to((1 << (np.arange(W) % B)).astype(np.uint16), shape)  # one bit per pixel, every position of a group
    pats = {"random": rng.integers(0, 1 << B, shape, dtype=np.uint16), "zero": np.zeros(shape, np.uint16),
            "ones": np.full(shape, (1 << B) - 1, np.uint16), "walking bit": np.ascontiguousarray(walk)}
    out = {}
    for k, c in pats.items():
        want = oracle.frontend.normalize_burst(c, BL, (1 << B) - 1, WB + [1.0], CFA)
        want.setflags(write=False)
        out[k] = (c, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", LAYOUTS)
def test_bit_exact(name, shape):
    """hhsr_normalize_raw_packed (called directly, with every stride / alignment) and utils_dng.normalize_packed ==
    oracle.frontend.normalize_burst(counts) == utils_dng.normalize_burst(counts), bit for bit; padding of every kind is
    0xFF; the NaN guard bands around `out` keep their bits."""
    B, (n, H, W) = BITS[name], shape
    wl = (1 << B) - 1
    need = table_row_bytes(W, name)
    guard = 64  # floats: out stays 16-byte aligned
    nan_bits = np.float32(np.nan).view(np.int32)
    cfa, bl, wb = _lib.cfa_bytes(CFA), _lib.doubles(BL), _lib.doubles(WB)
    for pat, (counts, want) in counts_and_reference(B, shape).items():
        u16 = utils_dng.normalize_burst(counts, BL, wl, WB, CFA).cpu().numpy()
        assert np.array_equal(u16, want), (name, shape, pat, "the uint16 path itself")
        for rb in (need, need + 3, -(-need // 16) * 16 + 16):
            for fb in (H * rb, H * rb + 7):
                for base in (0, 1):
                    buf, _, _ = pack_ff(counts, name, rb, fb, base)
                    dev = torch.from_numpy(buf).cuda()
                    big = torch.full((2 * guard + n * H * W,), float("nan"), dtype=torch.float32, device="cuda")
                    _lib.call("hhsr_normalize_raw_packed", ctypes.c_void_p(dev.data_ptr() + base), n, H, W, rb, fb,
                              utils_dng.PACKINGS[name], cfa, bl, float(wl), wb,
                              ctypes.c_void_p(big.data_ptr() + 4 * guard), _lib.stream())
                    got = big.cpu().numpy()
                    what = (name, shape, pat, rb, fb, base)
                    assert_close(got[guard:-guard].reshape(shape), want, 0, 0, "hhsr_normalize_raw_packed vs oracle normalize_burst")
                    assert np.array_equal(got[guard:-guard].reshape(shape), want), what
                    assert (got[:guard].view(np.int32) == nan_bits).all() and (got[-guard:].view(np.int32) == nan_bits).all(), what
            # the Python entry: compact frames [n, H, row_bytes], rows longer than their pixels included
            frames = pack_ff(counts, name, rb)[0].reshape(n, H, rb)
            got = utils_dng.normalize_packed(frames, W, name, BL, wl, WB, CFA)
            assert got.dtype == torch.float32 and tuple(got.shape) == shape
            assert_close(got.cpu().numpy(), want, 0, 0, "utils_dng.normalize_packed vs oracle normalize_burst")
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got.cpu().numpy(), u16), (name, shape, pat, rb)
        one = utils_dng.normalize_packed(torch.from_numpy(frames[0]), W, utils_dng.PACKINGS[name], BL, wl, WB, CFA)
        assert np.array_equal(one.cpu().numpy(), want[0])  # [H, row_bytes] -> [H, W]; a tensor; the layout by id
    with pytest.raises(TypeError):
        utils_dng.normalize_packed(frames.astype(np.uint16), W, name, BL, wl, WB, CFA)
    with pytest.raises(RuntimeError, match="invalid argument"):
        utils_dng.normalize_packed(frames[..., :need - 1], W, name, BL, wl, WB, CFA)


def small_config():
    """The configuration of test_hip_parity.test_process_integer_burst_and_monte_carlo_estimator."""
    c = hsr.default_config()
    c.verbose = 0
    c.block_matching.tuning.tile_size = 16
    c.block_matching.tuning.factors = [1, 2, 2, 2]
    c.block_matching.tuning.metrics = ["L2"] * 4
    return c


def burst_counts(B):
    """256 x 256 burst with 3 compared frames as B-bit counts whose normalisation is not the identity."""
    ref, comp, _ = synth.make_burst(256, 256, 3, seed=4)
    wb, wl = [1.8, 1.0, 1.4], (1 << B) - 1
    cfa = [[0, 1], [1, 2]]
    gains = np.array([[wb[cfa[i][j]] / wb[1] for j in range(2)] for i in range(2)], np.float64)
    g = np.tile(gains, (128, 128))
    to_counts = lambda x: np.clip(np.rint(x / g * (wl - 64) + 64), 0, wl).astype(np.uint16)  # noqa: E731
    return to_counts(ref), to_counts(comp), cfa, wb, [64, 64, 64], wl


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))  # (NaN border pixels included)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pad", [("mipi10", 0), ("be12", 16)])
def test_main_packed_frames(name, pad):
    """main() on pinned packed frames — eager, capture and replay of graph.HostBurstRunner with one configuration object —
    and on pageable NumPy packed frames == main() on the pinned uint16 counts, bit for bit; the ValueErrors of _ingest."""
    B = BITS[name]
    ref_c, comp_c, cfa, wb, bl, wl = burst_counts(B)
    stack = oracle.frontend.normalize_burst(ref_c, bl, wl, wb, cfa)
    W = ref_c.shape[1]
    rb = table_row_bytes(W, name) + pad
    pk = lambda c: pack_ff(c[None], name, rb)[0].reshape(c.shape[0], rb)  # noqa: E731
    ref_p, comp_p = pk(ref_c), [pk(c) for c in comp_c]

    def config(raw_norm=True, **keys):
        c = small_config()
        hsr.prepare_config(c, stack, synth.ALPHA_ISO100, synth.BETA_ISO100, cfa, wb)
        if raw_norm:
            c.hip = {"raw_norm": dict({"black_levels": bl, "white_level": wl}, **keys)}
        return c

    pin = lambda a: torch.from_numpy(a).pin_memory()  # noqa: E731
    want, _ = hsr.main(pin(ref_c), [pin(c) for c in comp_c], config())
    cp = config(packing=name, width=W)
    for call in ("eager", "capture", "replay"):
        got, _ = hsr.main(pin(ref_p), [pin(c) for c in comp_p], cp)
        assert_close(got.cpu().numpy(), want.cpu().numpy(), 0, 0, "main(packed frames) == main(uint16 counts)")
        assert same_bits(got, want), (name, call)
    # ... and the runner did capture (a failed capture falls back to the eager path, which gives the same bits): the
    # staging keeps the frames' own shape and dtype
    from handheld_super_resolution import super_resolution as sr

    runner = [r for c, _, r in sr._main_runners if c is cp][0]
    states = [st for st in runner.states.values() if st != "seen"]
    assert not runner.disabled and len(states) == 1, getattr(runner, "error", None)
    assert states[0].stage.dtype == torch.uint8 and tuple(states[0].stage.shape) == (1 + len(comp_p), ref_p.shape[0], rb)
    assert tuple(states[0].num.shape) == (round(cp.scale * ref_c.shape[0]), round(cp.scale * W), 3)  # the image is `width` wide
    got, _ = hsr.main(ref_p, comp_p, cp)  # pageable frames: the runner's copy threads
    assert same_bits(got, want), (name, "pageable")
    assert not runner.disabled and states[0].pin is not None and states[0].pin.dtype == torch.uint8
    with pytest.raises(ValueError, match="width"):
        hsr.main(pin(ref_p), [pin(c) for c in comp_p], config(packing=name))
    with pytest.raises(ValueError, match="width"):  # rows shorter than `width` pixels
        hsr.main(pin(ref_p), [pin(c) for c in comp_p], config(packing=name, width=W + 32))
    with pytest.raises(ValueError, match="packing"):
        hsr.main(pin(ref_p), [pin(c) for c in comp_p], config(packing="mipi8", width=W))
    with pytest.raises(ValueError, match="raw_norm"):  # integer frames without raw_norm, as before
        hsr.main(ref_p, comp_p, config(raw_norm=False))
    with pytest.raises(ValueError, match="raw_norm"):  # ... or already on the device
        hsr.main(torch.from_numpy(ref_p).cuda(), [torch.from_numpy(c).cuda() for c in comp_p], config(packing=name, width=W))


@pytest.mark.gpu
def test_process_packed_burst(tmp_path):
    """process() on a mapping with `packing` == process() on the uint16 counts: mipi10 with the width inferred from the
    rows, be12 with padded rows and an explicit width; the same bursts from an .npz file, where `packing` and `width`
    arrive as 0-d arrays."""
    meta = {"alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100}
    for name, pad in (("mipi10", 0), ("be12", 16)):
        ref_c, comp_c, cfa, wb, bl, wl = burst_counts(BITS[name])
        W = ref_c.shape[1]
        rb = table_row_bytes(W, name) + pad
        m = dict(meta, cfa_pattern=cfa, white_balance=wb, black_levels=bl, white_level=wl)
        want, _ = hsr.process(dict(m, ref=ref_c, comp=comp_c), small_config())
        packed = dict(m, ref=pack_ff(ref_c[None], name, rb)[0].reshape(-1, rb),
                      comp=pack_ff(comp_c, name, rb)[0].reshape(len(comp_c), -1, rb), packing=name)
        if pad:
            with pytest.raises(ValueError, match="width"):
                hsr.process(packed, small_config())  # 400-byte rows are no whole number of 12-bit pixels: no width to infer
            packed["width"] = W
        got, _ = hsr.process(packed, small_config())
        assert_close(got, want, 0, 0, f"process(packed {name}) == process(uint16 counts)")
        path = str(tmp_path / f"{name}.npz")
        np.savez(path, **packed)
        assert np.load(path)["packing"].shape == ()
        got, _ = hsr.process(path, small_config())
        assert_close(got, want, 0, 0, f"process(.npz, packed {name}) == process(uint16 counts)")
