"""Integer output without a GPU: the samples fixture of tests/output_ref.py, the PNG and TIFF writers parsed back with
struct and zlib alone, the argument refusals of hhsr_encode_image / hhsr_encode_mask, and the command line's
configuration."""
import ctypes
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import output_ref as ref

from handheld_super_resolution import _lib, utils_dng, utils_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 7), (3, 67)]


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_samples_fixture_holds_its_ties(bits):
    """Every float32((k + 0.5) / M) lands exactly on k + 0.5 after the float32 multiply, and for the even k rounding half
    up gives another sample than half to even: the counts are asserted so the fixture cannot quietly lose its ties."""
    M = ref.LEVELS[bits]
    s = ref.samples(bits)
    assert s.dtype == np.float32 and not s.flags.writeable
    k = np.arange(M)
    ties = s[-M:]
    assert np.array_equal(ties, ((k + 0.5) / M).astype(np.float32))
    p = ties * np.float32(M)
    assert p.dtype == np.float32
    assert int((p == k + 0.5).sum()) == M == {8: 255, 16: 65535}[bits]
    q = ref.quantize(ties, bits)
    half_up = np.floor(p.astype(np.float64) + 0.5).astype(q.dtype)
    assert int((q != half_up).sum()) == (M + 1) // 2 == {8: 128, 16: 32768}[bits]
    assert np.array_equal(q, k + (k & 1))  # half to even: k + 0.5 -> the even neighbour
    rest = s[:-M]
    assert np.isnan(rest).sum() == 1 and np.isposinf(rest).sum() == 1 and np.isneginf(rest).sum() == 1
    assert (np.signbit(rest) & (rest == 0)).sum() == 1                         # -0.0
    assert (rest < 0).sum() >= 3 and (rest > 1).sum() >= 3 and (rest == 1).sum() == 1
    assert np.nextafter(np.float32(1), np.float32(0)) in rest
    assert ((rest > 0) & (rest < np.finfo(np.float32).tiny)).sum() == 1        # a denormal
    want = {np.nan: 0, np.inf: M, -np.inf: 0, -0.0: 0, -5.0: 0, 2.0: M, 1.0: M, 1e-40: 0, 0.5: (M + 1) // 2}
    for x, y in want.items():
        assert int(ref.quantize(np.float32(x), bits)) == y, (x, y)
    assert int(ref.quantize(np.nextafter(np.float32(1), np.float32(0)), bits)) == M
    assert ref.quantize(s, bits).dtype == ref.DTYPES[bits]


def test_mask_reference_index_rule():
    acc = np.arange(12, dtype=np.float32).reshape(3, 4)
    m = ref.mask(acc, 11, (6, 8))  # integer ratio 2: every source pixel twice per axis
    assert m.dtype == np.uint8 and np.array_equal(m, np.repeat(np.repeat(ref.quantize(acc / np.float32(11), 8), 2, 0), 2, 1))
    m = ref.mask(acc, 11, (2, 5))
    assert np.array_equal(m, ref.quantize(acc / np.float32(11), 8)[[0, 1]][:, [0, 0, 1, 2, 3]])


# ---- the writers ------------------------------------------------------------------------------------------------------------
def image(shape, rgb, dtype, seed):
    rng = np.random.default_rng(seed)
    full = shape + (3,) if rgb else shape
    a = rng.integers(0, np.iinfo(dtype).max + 1, full).astype(dtype)
    a.flat[0] = np.iinfo(dtype).max
    a.flat[-1] = 0x0102 if dtype == np.uint16 else 0x01  # (byte order shows)
    return a


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_png_writer(tmp_path, shape, rgb, dtype):
    a = image(shape, rgb, dtype, 3)
    path = str(tmp_path / "a.png")
    utils_image.save_png(a, path)
    (W, H, depth, colour), px = ref.parse_png(path)
    assert (H, W) == shape and depth == 8 * a.dtype.itemsize and colour == (2 if rgb else 0)
    assert px.dtype == a.dtype and np.array_equal(px, a)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_tiff_writer(tmp_path, shape, rgb, dtype):
    a = image(shape, rgb, dtype, 4)
    path = tmp_path / "a.tif"
    utils_dng.save_as_tiff(a, path)
    tags, px = ref.parse_tiff(str(path))
    for t in (256, 257, 258, 259, 262, 273, 277, 278, 279, 284):
        assert t in tags, t
    assert (tags[257][2][0], tags[256][2][0]) == shape and tags[277][2] == ((3,) if rgb else (1,))
    assert px.dtype.itemsize == a.dtype.itemsize and np.array_equal(px, a)


def test_writers_refuse_what_they_cannot_hold(tmp_path):
    for bad in (np.zeros((2, 2), np.float32), np.zeros((2, 2, 4), np.uint8), np.zeros((2,), np.uint8), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError):
            utils_image.save_png(bad, str(tmp_path / "bad.png"))
        with pytest.raises(ValueError):
            utils_dng.save_as_tiff(bad, tmp_path / "bad.tif")
    utils_dng.save_as_tiff(np.zeros((2, 2), np.uint16), tmp_path / "named.dng")  # like upstream: the suffix becomes .tif
    assert (tmp_path / "named.tif").exists() and not (tmp_path / "named.dng").exists()


def test_png_round_trip_through_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for rgb in (False, True):
        a = image((5, 7), rgb, np.uint8, 5)
        path = str(tmp_path / "p.png")
        utils_image.save_png(a, path)
        with Image.open(path) as im:
            assert im.mode == ("RGB" if rgb else "L")
            assert np.array_equal(np.asarray(im), a)


def test_tiff_refuses_more_than_4_gib(tmp_path, monkeypatch):
    """Classic TIFF holds 32-bit offsets: the reference raises RuntimeError (utils_dng.py:335-341).  The size is faked."""
    a = np.zeros((2, 3, 3), np.uint16)
    monkeypatch.setattr(utils_dng, "_tiff_pixel_bytes", lambda arr: 2 ** 32 - 100)
    with pytest.raises(RuntimeError, match="too large"):
        utils_dng.save_as_tiff(a, tmp_path / "big.tif")
    assert not (tmp_path / "big.tif").exists()
    monkeypatch.setattr(utils_dng, "_tiff_pixel_bytes", lambda arr: 2 ** 32 - 1000)  # just below: accepted (the tag is the fake's)
    utils_dng.save_as_tiff(a, tmp_path / "big.tif")


# ---- argument refusals ------------------------------------------------------------------------------------------------------
def _pointers():
    """Two disjoint 16 MiB regions.  With a device: one zeroed tensor, far larger than what the valid calls below write (at
    most 64 x 96 x 3 uint16 with padded rows).  Without one nothing can launch: an arbitrary aligned address does."""
    import torch

    keep = torch.zeros(1 << 23, dtype=torch.float32, device="cuda") if torch.cuda.is_available() else None
    base = keep.data_ptr() if keep is not None else 1 << 32
    return keep, base, base + (1 << 24)


def test_encode_argument_refusals_do_not_touch_the_gpu():
    """Every refusal include/hhsr.h lists returns -1 with "invalid argument" before any HIP call; each is preceded by the same
    call with valid arguments, which must not return -1 (it launches on a device and fails in the runtime without one)."""
    lib = _lib.load()
    keep, img, out = _pointers()
    H, W = 64, 96
    P = ctypes.c_void_p
    valid = dict(image=img, H=H, W=W, channels=3, out_channels=3, out=out, bits=8, row=W * 3)

    def image_call(**kw):
        a = dict(valid, **kw)
        return lib.hhsr_encode_image(P(a["image"]), a["H"], a["W"], a["channels"], a["out_channels"], P(a["out"]), a["bits"],
                                     a["row"], None)

    missed = []

    def refused(call, **kw):
        rc = call(**kw)
        if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
            missed.append((call.__name__, kw, rc, lib.hhsr_last_error()))

    u16 = dict(bits=16, row=W * 6)
    grey = dict(out_channels=1, row=W)
    image_refusals = [  # (a valid variant of the call, what is then made wrong)
        ({}, dict(image=None)), ({}, dict(out=None)),                                    # null pointers
        ({}, dict(bits=12)), ({}, dict(bits=0)), (u16, dict(bits=32)),                   # bits not in {8, 16}
        ({}, dict(channels=2, out_channels=2)), (grey, dict(channels=4)), ({}, dict(channels=0, out_channels=0)),
        ({}, dict(out_channels=2)), (dict(channels=1, out_channels=1, row=W * 3), dict(out_channels=3)),
        ({}, dict(row=W * 3 - 1)), (u16, dict(row=W * 6 - 2)), (grey, dict(row=W - 1)),  # a short row stride
        (u16, dict(out=out + 1)), ({}, dict(image=img + 2)),                             # a pointer off its samples' alignment
        ({}, dict(out=img)), ({}, dict(out=img + H * W * 12 - 1)), ({}, dict(image=out + 8)),  # out overlapping image
        ({}, dict(H=0)), ({}, dict(W=0)), ({}, dict(H=-1)),
    ]
    for ok, bad in image_refusals:
        assert image_call(**ok) >= 0, (ok, lib.hhsr_last_error())
        refused(image_call, **dict(ok, **bad))
    assert image_call(out=img + H * W * 12) >= 0  # out directly behind image: no overlap
    assert image_call(out=out + 3, row=W * 3 + 5) >= 0 and image_call(bits=16, out=out + 2, row=W * 6 + 2) >= 0
    assert image_call(bits=16, row=W * 6 + 1) >= 0  # an odd stride of 16-bit rows is served (byte by byte), not refused
    # a sample count the launch cannot hold: one workgroup per 4096 output bytes, at most INT32_MAX of them (nothing is
    # dereferenced before the refusal, the pointers are far apart); so large that the byte counts overflow: refused too.
    # C5's output, 18000 x 24000 x 3 samples, is far inside the limit at both widths.
    apart = dict(image=img, out=img + (1 << 60)) if keep is None else {}  # (on a device the valid call launches: real memory)
    assert image_call(**apart) >= 0, lib.hhsr_last_error()
    refused(image_call, image=1 << 12, out=1 << 60, H=1 << 21, W=1 << 21, row=3 << 21)
    assert image_call(bits=16, row=W * 6, **apart) >= 0, lib.hhsr_last_error()
    refused(image_call, image=1 << 12, out=1 << 60, H=INT_MAX, W=INT_MAX, bits=16, row=INT_MAX * 6)
    assert -(-(18000 * 24000 * 3 * 2) // 4096) < INT_MAX // 1000

    mvalid = dict(acc=img, ah=8, aw=12, n=2, out=out, mH=16, mW=24, row=24)

    def mask_call(**kw):
        a = dict(mvalid, **kw)
        return lib.hhsr_encode_mask(P(a["acc"]), a["ah"], a["aw"], a["n"], ctypes.cast(P(a["out"]), _lib.U8P), a["mH"], a["mW"],
                                    a["row"], None)

    for kw in (dict(acc=None), dict(out=None), dict(ah=0), dict(aw=0), dict(mH=0), dict(mW=-3), dict(n=0), dict(n=-1),
               dict(row=23), dict(acc=img + 1), dict(out=img + 4), dict(acc=out, out=out + 8 * 12 * 4 - 1)):
        assert mask_call() >= 0, lib.hhsr_last_error()
        refused(mask_call, **kw)
    assert mask_call(out=out + 1, row=29) >= 0
    if keep is not None:
        import torch

        torch.cuda.synchronize()
    assert not missed, missed


INT_MAX = 2 ** 31 - 1


# ---- command line -----------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location(
        "hhsr_run_handheld", os.path.join(ROOT, "handheld-multi-frame-super-resolution_amd", "run_handheld.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_refuses_dng_and_names_the_tools():
    cli = _cli()
    with pytest.raises(NotImplementedError, match=r"exiftool.*dng_validate"):
        cli.main(["--impath", "burst.npz", "--outpath", "out.dng"])
    with pytest.raises(ValueError):
        cli.build_config(cli.parse_args(["--impath", "burst.npz", "--outpath", "out.jpg"]))


def test_command_line_overrides_reach_the_configuration(tmp_path):
    cli = _cli()
    yml = tmp_path / "user.yaml"
    yml.write_text("scale: 3\nica:\n  tuning:\n    n_iter: 5\n")
    cfg = cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", "o.png", "--config", str(yml), "scale=2",
                                           "robustness.save_mask=false", "merging.kernel=iso",
                                           "block_matching.tuning.factors=[1, 2, 2, 2]", "robustness.tuning.t=0.25",
                                           "debug=__import__('os').getcwd()"]))
    assert cfg.scale == 2 and cfg.ica.tuning.n_iter == 5 and cfg.ica.tuning.sigma_blur == 0  # override > file > defaults
    assert cfg.robustness.save_mask is False and cfg.merging.kernel == "iso" and cfg.robustness.tuning.t == 0.25
    assert cfg.block_matching.tuning.factors == [1, 2, 2, 2] and cfg.robustness.tuning.s1 == 2
    assert cfg.debug == "__import__('os').getcwd()"  # a string stays a string: nothing is evaluated
    assert cfg.output.dtype == "uint8"
    for name, want in (("o.tif", "uint16"), ("o.TIFF", "uint16"), ("o.PNG", "uint8")):
        assert cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", name])).output.dtype == want
    with pytest.raises(ValueError):
        cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", "o.png", "scale"]))
    with pytest.raises(ValueError, match="both or neither"):  # half a noise profile
        cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", "o.png", "noise_model.alpha=0.001"]))
    both = cli.build_config(cli.parse_args(["--impath", "b.npz", "--outpath", "o.png", "noise_model.alpha=0.001",
                                            "noise_model.beta=0.00001"]))
    assert both.noise_model.alpha == 0.001 and both.noise_model.beta == 1e-5
