"""Integer output on the GPU: hhsr_encode_image and hhsr_encode_mask against the NumPy restatement tests/output_ref.py,
process() with config.output, and the command line end to end.  Every comparison is of integer images, at tolerance 0.

Every output buffer is pre-filled with 0xA5 and carries 256 bytes of guard behind (and, with an offset base, the offset's
bytes in front of) the image: bytes that are no sample — row padding, guard, offset — must still hold 0xA5."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import output_ref as ref
from helpers import assert_close

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, synthetic as synth, utils_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, GUARD = 0xA5, 256
SHAPES = [(1, 1), (1, 5), (3, 67), (37, 261), (1201, 1603)]  # the last: more than one round of workgroups
CHANNELS = [(3, 3), (3, 1), (1, 1)]


@functools.lru_cache(maxsize=None)
def case(shape, ch, och, bits):
    """(input float32 image, expected samples [H, W * och]) — computed once, shared, read-only."""
    img = ref.make_image(shape, ch, bits, seed=shape[0] * 31 + shape[1] + ch + bits)
    src = img[..., 0] if (ch == 3 and och == 1) else img
    want = ref.quantize(src, bits).reshape(shape[0], -1)
    img.setflags(write=False)
    want.setflags(write=False)
    return img, want


def run_encode(img, och, bits, row_bytes=None, base=0):
    """hhsr_encode_image into a guarded 0xA5 buffer -> (samples [H, W * och], every byte that is no sample)."""
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    bps = bits // 8
    need = W * och * bps
    rb = need if row_bytes is None else row_bytes
    span = (H - 1) * rb + need
    buf = torch.full((base + span + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    src = torch.tensor(img).cuda()
    _lib.call("hhsr_encode_image", _lib.ptr(src), H, W, ch, och, buf.data_ptr() + base, bits, rb, _lib.stream())
    got = buf.cpu().numpy()
    idx = base + np.arange(H)[:, None] * rb + np.arange(need)[None, :]
    rows = np.ascontiguousarray(got[idx])
    other = np.ones(got.size, bool)
    other[idx.ravel()] = False
    return (rows.view("<u2") if bits == 16 else rows), got[other]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ch,och", CHANNELS)
@pytest.mark.parametrize("bits", [8, 16])
def test_encode_image_matches_reference(bits, ch, och, shape):
    img, want = case(shape, ch, och, bits)
    got, other = run_encode(img, och, bits)
    assert got.dtype == want.dtype
    assert_close(got, want, 0, 0, what=f"hhsr_encode_image {bits} bits, {ch} -> {och} channels, {shape[0]}x{shape[1]}")
    assert other.size == GUARD and (other == FILL).all(), "bytes behind the image were written"


@pytest.mark.parametrize("shape", [(3, 67), (37, 261)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ch,och", CHANNELS)
@pytest.mark.parametrize("pad", [1, 7, 64])
@pytest.mark.parametrize("bits,base", [(8, 0), (8, 1), (8, 2), (8, 3), (16, 0), (16, 2)])
def test_encode_image_padded_rows_and_offset_bases(bits, base, pad, ch, och, shape):
    """Rows out_row_bytes apart, from a base that is aligned to the sample size only: the compact result, and the bytes
    between the rows, in front of the base and behind the image keep their 0xA5.  (needed + 1 and + 7 put every other row
    of 16-bit samples on an odd byte.)"""
    img, want = case(shape, ch, och, bits)
    need = shape[1] * och * bits // 8
    got, other = run_encode(img, och, bits, row_bytes=need + pad, base=base)
    assert_close(got, want, 0, 0, what=f"hhsr_encode_image padded rows, {bits} bits, {ch} -> {och}, + {pad}, base {base}")
    assert other.size == base + (shape[0] - 1) * pad + GUARD and (other == FILL).all(), "padding or guard bytes were written"
    if pad == 1:  # an offset base alone, compact rows: one run from an unaligned start
        got, other = run_encode(img, och, bits, base=base)
        assert_close(got, want, 0, 0, what=f"hhsr_encode_image compact, {bits} bits, {ch} -> {och}, base {base}")
        assert other.size == base + GUARD and (other == FILL).all()


@pytest.mark.parametrize("pad", [1, 64])
@pytest.mark.parametrize("bits,base", [(8, 0), (8, 3), (16, 0), (16, 2)])
def test_encode_image_padded_rows_longer_than_a_workgroup(bits, base, pad):
    """Rows of 1603 x 3 samples — 4809 / 9618 bytes, two / three workgroups of 4096 bytes each — with padding: several runs
    of several tiles in one launch (the workgroup -> (row, tile) split; with + 1 at 16 bits the byte-by-byte rows' tiles)."""
    shape = (5, 1603)
    img, want = case(shape, 3, 3, bits)
    need = shape[1] * 3 * bits // 8
    assert need > 4096
    got, other = run_encode(img, 3, bits, row_bytes=need + pad, base=base)
    assert_close(got, want, 0, 0, what=f"hhsr_encode_image padded rows of {need} bytes, {bits} bits, + {pad}, base {base}")
    assert other.size == base + (shape[0] - 1) * pad + GUARD and (other == FILL).all(), "padding or guard bytes were written"


MASKS = [((8, 12), (16, 24)), ((8, 12), (12, 18)), ((7, 9), (21, 27)), ((8, 12), (8, 12)), ((5, 7), (13, 10))]


@pytest.mark.parametrize("src,dst", MASKS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n_comp", [1, 3])
def test_encode_mask_matches_reference(n_comp, src, dst):
    rng = np.random.default_rng(src[0] * 100 + dst[1] + n_comp)
    acc = rng.uniform(0, 1.25 * n_comp, src).astype(np.float32)  # a fifth of the values above n_comp
    acc.flat[:: 7] = np.resize(np.array([np.nan, 0.5 * n_comp, n_comp, 2.0 * n_comp, 0.0, -1.0, np.inf], np.float32),
                               acc.flat[:: 7].size)
    assert np.isnan(acc).any() and (acc > n_comp).any()
    want = ref.mask(acc, n_comp, dst)
    mH, mW = dst
    dev = torch.from_numpy(acc).cuda()
    assert_close(utils_image.robustness_mask(dev, n_comp, dst).cpu().numpy(), want, 0, 0,
                 what=f"robustness_mask {src} -> {dst}, n_comp {n_comp}")
    for base, rb in ((0, mW), (1, mW + 5), (3, mW + 64)):
        buf = torch.full((base + (mH - 1) * rb + mW + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        _lib.call("hhsr_encode_mask", _lib.ptr(dev), src[0], src[1], n_comp, buf.data_ptr() + base, mH, mW, rb, _lib.stream())
        got = buf.cpu().numpy()
        idx = base + np.arange(mH)[:, None] * rb + np.arange(mW)[None, :]
        assert_close(got[idx], want, 0, 0, what=f"hhsr_encode_mask {src} -> {dst}, n_comp {n_comp}, base {base}, row {rb}")
        other = np.ones(got.size, bool)
        other[idx.ravel()] = False
        assert (got[other] == FILL).all(), "padding or guard bytes were written"


def test_encode_image_python_wrapper():
    img, _ = case((37, 261), 3, 3, 8)
    dev = torch.tensor(img).cuda()
    for name, bits in (("uint8", 8), ("uint16", 16)):
        full = utils_image.encode_image(dev, name)
        assert full.is_cuda and full.dtype == getattr(torch, name) and tuple(full.shape) == img.shape
        assert_close(full.cpu().numpy(), ref.quantize(img, bits), 0, 0, what=f"encode_image {name}")
        grey = utils_image.encode_image(dev, getattr(torch, name), channels=1)
        assert tuple(grey.shape) == img.shape[:2]
        assert_close(grey.cpu().numpy(), ref.quantize(img[..., 0], bits), 0, 0, what=f"encode_image {name}, channel 0")
        view = dev.transpose(0, 1).flip(1)  # a strided view: copied first
        assert_close(utils_image.encode_image(view, np.dtype(name)).cpu().numpy(),
                     ref.quantize(np.flip(img.transpose(1, 0, 2), 1), bits), 0, 0, what=f"encode_image {name}, strided view")
    with pytest.raises(ValueError):
        utils_image.encode_image(dev, "int8")
    with pytest.raises(ValueError):
        utils_image.encode_image(dev, "uint8", channels=2)
    with pytest.raises(RuntimeError):
        utils_image.encode_image(torch.tensor(img), "uint8")


# ---- process() ----------------------------------------------------------------------------------------------------------------
OVERRIDES = ["verbose=0", "scale=2", "block_matching.tuning.tile_size=16", "block_matching.tuning.factors=[1, 2, 2, 2]",
             "block_matching.tuning.metrics=[L2, L2, L2, L2]"]


@functools.lru_cache(maxsize=None)
def burst():
    ref_raw, comp, _ = synth.make_burst(128, 160, 3, seed=21, max_shift=1.5)
    std, diff = synth.noise_curves(synth.ALPHA_ISO100, synth.BETA_ISO100)
    return {"ref": ref_raw, "comp": comp, "cfa_pattern": np.array([[0, 1], [1, 2]]), "white_balance": np.ones(3),
            "alpha": synth.ALPHA_ISO100, "beta": synth.BETA_ISO100, "std_curve": std, "diff_curve": diff, "orientation": 6}


def processed(dtype, post=True, mode="bayer", save_mask=True):
    """process() of the burst at x2, once per configuration.  dtype None: no `output` section at all."""
    return _processed(dtype, post, mode, save_mask)


@functools.lru_cache(maxsize=None)
def _processed(dtype, post, mode, save_mask):
    cfg = hsr.default_config()
    cfg.verbose = 0
    cfg.scale = 2
    cfg.mode = mode
    cfg.block_matching.tuning.tile_size = 16
    cfg.block_matching.tuning.factors = [1, 2, 2, 2]
    cfg.block_matching.tuning.metrics = ["L2"] * 4
    cfg.postprocessing.enabled = post
    cfg.robustness.save_mask = save_mask
    if dtype is not None:
        cfg.output = {"dtype": dtype}
    img, dbg = hsr.process(dict(burst()), cfg)
    img.setflags(write=False)
    return img, dbg


@pytest.mark.parametrize("post", [True, False], ids=["post_on", "post_off"])
@pytest.mark.parametrize("dtype,bits", [("uint8", 8), ("uint16", 16)])
def test_process_integer_output(dtype, bits, post):
    f32, _ = processed(None, post)
    got, dbg = processed(dtype, post)
    assert f32.dtype == np.float32 and f32.shape == (320, 256, 3)  # orientation 6: [sW][sH][3]
    assert got.dtype == np.dtype(dtype) and got.shape == f32.shape
    assert_close(got, ref.quantize(f32, bits), 0, 0, what=f"process() {dtype}, postprocessing {'on' if post else 'off'}")
    assert got.min() < got.max()
    assert dbg["accumulated robustness"].dtype == np.float32  # stays as it is


def test_process_grey_mode_is_one_channel():
    f32, _ = processed(None, True, "grey")
    assert f32.shape == (320, 256, 3) and np.isnan(f32[..., 1:]).all()
    for dtype, bits in (("uint8", 8), ("uint16", 16)):
        got, _ = processed(dtype, True, "grey")
        assert got.dtype == np.dtype(dtype) and got.shape == (320, 256)
        assert_close(got, ref.quantize(f32[..., 0], bits), 0, 0, what=f"process() {dtype}, mode grey")


def test_process_robustness_mask():
    got, dbg = processed("uint8")
    acc = dbg["accumulated robustness"]
    assert acc.shape == (160, 128) and "robustness mask" in dbg  # oriented, at the raw frame's size
    m = dbg["robustness mask"]
    assert m.dtype == np.uint8 and m.shape == got.shape[:2]
    assert_close(m, ref.mask(acc, 2, got.shape[:2]), 0, 0, what="process() robustness mask")
    assert "robustness mask" not in processed("uint8", True, "bayer", False)[1]  # save_mask off: no mask
    assert "robustness mask" not in processed(None)[1]                            # float32 output: as before


def test_process_float32_is_unchanged():
    a, da = processed(None)
    b, db = processed("float32")
    assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert sorted(da) == sorted(db) and da["accumulated robustness"].tobytes() == db["accumulated robustness"].tobytes()
    cfg = hsr.default_config()
    cfg.output = {"dtype": "int16"}
    with pytest.raises(ValueError, match="output.dtype"):
        hsr.process(dict(burst()), cfg)


# ---- command line -------------------------------------------------------------------------------------------------------------
def run_cli(tmp_path, outname, *overrides):
    npz = tmp_path / "burst.npz"
    if not npz.exists():
        np.savez(npz, **burst())
    out = tmp_path / outname
    cli = os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd", "run_handheld.py")
    r = subprocess.run([sys.executable, cli, "--impath", str(npz), "--outpath", str(out), *OVERRIDES, *overrides],
                       capture_output=True, text=True, timeout=180)  # a fresh child process
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out


def test_command_line_end_to_end(tmp_path):
    out = run_cli(tmp_path, "result.png", "robustness.save_mask=true")
    want, dbg = processed("uint8")
    (W, H, depth, colour), px = ref.parse_png(str(out))
    assert (depth, colour) == (8, 2)
    assert_close(px, want, 0, 0, what="run_handheld.py .png")
    (W, H, depth, colour), px = ref.parse_png(str(tmp_path / "result.rob.png"))
    assert (depth, colour) == (8, 0)
    assert_close(px, dbg["robustness mask"], 0, 0, what="run_handheld.py .rob.png")

    out = run_cli(tmp_path, "result.tif", "robustness.save_mask=false")
    assert not (tmp_path / "result.rob.tif").exists() and sorted(os.listdir(tmp_path)) == [
        "burst.npz", "result.png", "result.rob.png", "result.tif"]
    tags, px = ref.parse_tiff(str(out))
    assert tags[258][2] == (16, 16, 16)
    assert_close(px, processed("uint16")[0], 0, 0, what="run_handheld.py .tif")
