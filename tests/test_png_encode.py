"""PNG output on the GPU: hhsr_png_filter and hhsr_png_deflate against the restatement tests/png_ref.py, encode_png's files,
and process() with output.format = png.  Everything is compared at tolerance 0: the file's bytes are a function of the image
and the options.

Every device buffer a call writes (filtered stream, counts, scratch, deflate stream, result words) lies between two 0xA5
guard bands of 256 bytes, and the bands are checked after every call."""
import ctypes as C
import functools
import importlib.util
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_ref as ref
import test_jpeg_encode as base  # the burst, the configuration and the cached process() calls of the JPEG tests

import handheld_super_resolution as hsr
from handheld_super_resolution import _lib, utils_image

pytestmark = pytest.mark.gpu

Guarded = base.Guarded
# (1, 1) .. (136, 264) as for JPEG; (3, 5000): a row of more than one 4096-sample segment of the filter kernel (two grey,
# four RGB); (1100, 3): more rows than the filter kernel has workgroups (1024)
SHAPES = [(1, 1), (1, 64), (64, 1), (2, 3), (9, 17), (40, 72), (136, 264), (3, 5000), (1100, 3)]
LAYOUTS = [(1, 1), (3, 3), (3, 1)]  # (channels of the image, channels of the file)
KINDS = ["random", "smooth", "constant", "wild"]


def gpu_filter(img, och, bits, filt):
    """hhsr_png_filter of a float32 ndarray -> (the filtered stream uint8 [N], counts uint64 [256])."""
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    n, scratch_bytes, _ = utils_image.png_workspace(H, W, och, bits, 1 << 20)
    src = torch.tensor(img).cuda()
    stream, counts, scratch = Guarded(n), Guarded(2048), Guarded(scratch_bytes)
    _lib.call("hhsr_png_filter", _lib.ptr(src), H, W, ch, och, bits, filt, stream.ptr, n, counts.ptr, scratch.ptr,
              scratch_bytes, _lib.stream())
    scratch.read()
    return stream.read().copy(), counts.read().view(np.uint64).copy()


def gpu_deflate(stream, interval, spec, capacity=None):
    """hhsr_png_deflate of a uint8 ndarray -> (the first min(length, capacity) bytes, the three result words, the whole
    output buffer).  capacity None: a true bound for any stream of this length."""
    n = stream.size
    n_int = ref.n_intervals(n, interval)
    scratch_bytes = 24 * n_int + 8 * -(-n_int // 2048)
    cap = n * 2 + 480 * n_int if capacity is None else capacity
    dev = torch.tensor(np.ascontiguousarray(stream, np.uint8)).cuda()
    scratch, out, result = Guarded(scratch_bytes), Guarded(cap), Guarded(24)
    _lib.call("hhsr_png_deflate", _lib.ptr(dev), n, interval, spec.ctypes.data_as(C.POINTER(C.c_uint8)), scratch.ptr,
              scratch_bytes, out.ptr, cap, result.ptr, _lib.stream())
    scratch.read()
    words = [int(v) for v in result.read().view(np.uint64)]
    whole = out.read()
    return whole[:min(words[0], cap)].tobytes(), words, whole


def spec_for(stream, interval):
    counts = np.zeros(257, np.uint64)
    counts[:256] = ref.byte_counts(stream)
    counts[256] = ref.n_intervals(stream.size, interval)
    return utils_image.png_huffman(counts)


@functools.lru_cache(maxsize=None)
def image(shape, channels, kind):
    return ref.test_images(shape[0], shape[1], channels, seed=shape[0] * 7 + shape[1] + channels)[kind]


def reference_stream(img, och, bits, filt):
    rows, bpp = ref.row_bytes(ref.samples(img, bits, channels=1 if och == 1 else None))
    return ref.filtered_stream(rows, bpp, filt)


# ---- 1. filtered stream and counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ch,och", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_filtered_stream_and_counts(shape, ch, och, bits):
    for kind in KINDS:
        img = image(shape, ch, kind)
        for filt in range(6):
            want, _ = reference_stream(img, och, bits, filt)
            got, counts = gpu_filter(img, och, bits, filt)
            assert np.array_equal(got, want), (kind, filt, np.flatnonzero(got != want)[:8])
            assert np.array_equal(counts, ref.byte_counts(want)), (kind, filt)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ch,och", LAYOUTS)
def test_filter_none_is_encode_image(ch, och, bits):
    img = image((40, 72), ch, "wild")
    got, _ = gpu_filter(img, och, bits, 0)
    q = utils_image.encode_image(torch.tensor(img).cuda(), "uint8" if bits == 8 else "uint16",
                                 channels=1 if och != ch else None).cpu().numpy()
    rows, _ = ref.row_bytes(q)
    got = got.reshape(40, -1)
    assert not got[:, 0].any() and np.array_equal(got[:, 1:], rows)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("channels,W", [(1, 37), (3, 37), (1, 64), (3, 64)])
def test_adaptive_choice_picks_every_type(channels, W, bits):
    img = ref.five_filter_image(W, channels)
    want, types = reference_stream(img, channels, bits, 5)
    assert sorted(set(int(t) for t in types)) == [0, 1, 2, 3, 4], types  # (of the reference: all five occur in this image)
    got, counts = gpu_filter(img, channels, bits, 5)
    assert np.array_equal(got, want) and np.array_equal(counts, ref.byte_counts(want))


def test_filter_of_an_unaligned_image():
    """An image that is 4-byte but not 16-byte aligned takes the scalar loads."""
    img = image((9, 17), 3, "random")
    buf = torch.zeros(img.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.tensor(img).reshape(-1)
    src = buf[1:]
    assert src.data_ptr() % 16 == 4
    n, scratch_bytes, _ = utils_image.png_workspace(9, 17, 3, 8, 4096)
    stream, counts, scratch = Guarded(n), Guarded(2048), Guarded(scratch_bytes)
    _lib.call("hhsr_png_filter", _lib.ptr(src), 9, 17, 3, 3, 8, 5, stream.ptr, n, counts.ptr, scratch.ptr, scratch_bytes,
              _lib.stream())
    want, _ = reference_stream(img, 3, 8, 5)
    assert np.array_equal(stream.read(), want) and np.array_equal(counts.read().view(np.uint64), ref.byte_counts(want))


# ---- 2. deflate -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def byte_stream(name):
    """Streams for the coder alone (it takes any bytes): a real filtered stream; 21 values with Fibonacci counts, whose
    optimal code reaches the 15-bit limit, of a length that is no multiple of 4; all 256 values."""
    rng = np.random.default_rng(17)
    if name == "filtered":
        return reference_stream(image((40, 72), 3, "smooth"), 3, 8, 5)[0]            # 8680 bytes
    if name == "fibonacci":
        fib = [1, 2]
        while len(fib) < 21:
            fib.append(fib[-1] + fib[-2])
        values = np.repeat(np.arange(21) * 12, fib).astype(np.uint8)[:-1]                # 28655 bytes
        rng.shuffle(values)
        return values
    return rng.integers(0, 256, 3001).astype(np.uint8)


def check_deflate(stream, interval, inflate=True):
    spec = spec_for(stream, interval)
    want = ref.deflate(stream, interval, spec)
    got, (length, crc, adler), _ = gpu_deflate(stream, interval, spec)
    assert length == len(want)
    assert got == want, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
    assert crc == zlib.crc32(want) and adler == zlib.adler32(stream.tobytes())
    if inflate:  # (of the reference: the layout inflates)
        assert zlib.decompress(want, wbits=-15) == stream.tobytes()


# a wave's pass is 1024 bytes, 16 per lane.  1: one byte per interval; 7, 1000: no multiple of the lanes' 16; 300 < one pass <
# 1500 and 2500 (the last pass 452 bytes: lanes without a byte); 1024, 2048: whole passes; N - 1: a last interval of 1 byte;
# N and 2^20: one interval for everything
@pytest.mark.parametrize("interval", [1, 7, 300, 1000, 1024, 1025, 1500, 2048, 2500, "N-1", "N", 1 << 20])
@pytest.mark.parametrize("name", ["filtered", "fibonacci", "uniform"])
def test_deflate_bytes_and_result_words(name, interval):
    stream = byte_stream(name)
    n = stream.size
    check_deflate(stream, {"N-1": n - 1, "N": n}.get(interval, interval))
    if name == "fibonacci" and interval == 300:
        assert stream.size % 4 != 0 and ref.spec_parts(spec_for(stream, 300))[0].max() == 15  # (it does reach the longest code)


def test_deflate_crosses_every_boundary_of_the_offsets_scan():
    """One-byte intervals: 600 000 of them are more than 256 groups of 2048 intervals — the scan's second level walks the
    groups 256 at a time — so every boundary of the scan is crossed: thread, wave, workgroup, group of groups."""
    rng = np.random.default_rng(23)
    stream = np.minimum(rng.geometric(0.3, 600_000) - 1, 255).astype(np.uint8)
    assert stream.size > 256 * 2048
    check_deflate(stream, 1, inflate=False)


def test_deflate_more_intervals_than_waves():
    """More than 2^20 intervals: the waves walk the intervals by stride."""
    rng = np.random.default_rng(29)
    stream = np.minimum(rng.geometric(0.5, (1 << 20) + 777) - 1, 255).astype(np.uint8)
    check_deflate(stream, 1, inflate=False)


def test_deflate_missing_symbol_is_reported():
    stream = byte_stream("uniform")
    spec = spec_for(np.where(stream == 7, 8, stream).astype(np.uint8), 300)  # a code without the value 7
    assert ref.spec_parts(spec)[0][7] == 0 and (stream == 7).any()
    _, (length, _, _), _ = gpu_deflate(stream, 300, spec)
    assert length == (1 << 64) - 1


# ---- 3. whole files -----------------------------------------------------------------------------------------------------------------
def reference_file(img, och, bits, filt, interval):
    H, W = img.shape[:2]
    stream, _ = reference_stream(img, och, bits, filt)
    return ref.png_file(H, W, och, bits, stream, interval, spec_for(stream, interval)), stream


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ch,och", LAYOUTS)
@pytest.mark.parametrize("shape", [(1, 1), (9, 17), (40, 72), (3, 5000)])
def test_whole_files(shape, ch, och, bits):
    from PIL import Image

    for kind, filt, interval in (("random", "adaptive", 300), ("smooth", "adaptive", None), ("wild", "paeth", 4096),
                                 ("constant", "none", 1 << 20)):
        img = image(shape, ch, kind)
        dev = torch.tensor(img).cuda()
        data = utils_image.encode_png(dev, bits=bits, channels=1 if och != ch else None, filter=filt, interval_bytes=interval)
        assert data.dtype == np.uint8 and data.ndim == 1
        want, stream = reference_file(img, och, bits, utils_image.PNG_FILTERS[filt],
                                      utils_image.PNG_INTERVAL_BYTES if interval is None else interval)
        assert data.tobytes() == want, (kind, filt, interval)
        H, W, c, b, payload = ref.parse(data)
        assert (H, W, c, b) == (*shape, och, bits) and zlib.decompress(payload) == stream.tobytes()
        q = utils_image.encode_image(dev, "uint8" if bits == 8 else "uint16", channels=1 if och != ch else None).cpu().numpy()
        if och == 3 and bits == 16:  # Pillow reduces 16-bit RGB to 8 bits: the restatement's unfilter instead
            back = ref.decode(data) if img.size <= 40 * 72 * 3 else None
        else:
            back = np.asarray(Image.open(io.BytesIO(data.tobytes())))
        if back is not None:
            assert back.dtype == q.dtype and np.array_equal(back, q), (kind, filt)


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 1, 3, 1000, "n-1", "n"])
def test_capacity_is_respected(capacity):
    stream = byte_stream("filtered")
    spec = spec_for(stream, 300)
    want = ref.deflate(stream, 300, spec)
    cap = {"n-1": len(want) - 1, "n": len(want)}.get(capacity, capacity)
    got, (length, crc, adler), whole = gpu_deflate(stream, 300, spec, capacity=cap)  # (Guarded checks the bands behind cap)
    assert length == len(want) and got == want[:cap]
    assert crc == zlib.crc32(want) and adler == zlib.adler32(stream.tobytes())  # of the whole stream, whatever fitted


def test_encode_png_retries_once():
    dev = torch.tensor(image((40, 72), 3, "smooth")).cuda()
    want = utils_image.encode_png(dev, interval_bytes=300)
    for cap in (0, 10, want.size - 64):
        assert utils_image.encode_png(dev, interval_bytes=300, capacity=cap).tobytes() == want.tobytes()


# ---- 5. reproducibility -----------------------------------------------------------------------------------------------------------------
def test_bytes_do_not_depend_on_the_run_or_the_stream():
    dev = torch.tensor(image((136, 264), 3, "smooth")).cuda()
    first = utils_image.encode_png(dev, bits=16, interval_bytes=1000)
    assert utils_image.encode_png(dev, bits=16, interval_bytes=1000).tobytes() == first.tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = utils_image.encode_png(dev, bits=16, interval_bytes=1000)
    side.synchronize()
    assert other.tobytes() == first.tobytes()


# ---- 6. process() and the command line ---------------------------------------------------------------------------------------------------
def test_process_returns_the_file():
    f32, _ = base.processed(None)
    u8, dbg8 = base.processed((("dtype", "uint8"),))
    png, dbg = base.processed((("format", "png"),))
    assert png.dtype == np.uint8 and png.ndim == 1 and ref.parse(png)[:4] == (320, 256, 3, 8)
    assert png.tobytes() == utils_image.encode_png(torch.tensor(f32).cuda()).tobytes()
    assert np.array_equal(ref.decode(png), u8)
    assert dbg["robustness mask"].dtype == np.uint8 and np.array_equal(dbg["robustness mask"], dbg8["robustness mask"])
    assert dbg["accumulated robustness"].tobytes() == dbg8["accumulated robustness"].tobytes()
    opt, _ = base.processed((("format", "png"), ("dtype", "uint8"), ("filter", "up"), ("interval_bytes", 5000)))
    assert opt.tobytes() == utils_image.encode_png(torch.tensor(f32).cuda(), filter="up", interval_bytes=5000).tobytes()


def test_process_honours_uint16_and_grey_mode():
    from PIL import Image

    f32, _ = base.processed(None)
    png16, _ = base.processed((("format", "png"), ("dtype", "uint16")))
    assert ref.parse(png16)[:4] == (320, 256, 3, 16)
    assert png16.tobytes() == utils_image.encode_png(torch.tensor(f32).cuda(), bits=16).tobytes()
    g32, _ = base.processed(None, "grey")
    for dtype, bits in (("uint8", 8), ("uint16", 16)):
        grey, _ = base.processed((("format", "png"), ("dtype", dtype)), "grey")
        assert ref.parse(grey)[:4] == (320, 256, 1, bits)
        assert grey.tobytes() == utils_image.encode_png(torch.tensor(g32).cuda(), bits=bits, channels=1).tobytes()
        want = utils_image.encode_image(torch.tensor(g32).cuda(), dtype, channels=1).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(grey.tobytes()))), want)


def test_process_without_format_png_is_unchanged():
    """The calls of tests/test_jpeg_encode.py: format absent, raw and jpeg give what they gave."""
    f32, d32 = base.processed(None)
    for out in ((("format", "raw"),), (("format", "raw"), ("dtype", "float32"))):
        got, dbg = base.processed(out)
        assert got.dtype == np.float32 and got.tobytes() == f32.tobytes() and sorted(dbg) == sorted(d32)
    u8, _ = base.processed((("dtype", "uint8"),))
    got, _ = base.processed((("dtype", "uint8"), ("format", "raw")))
    assert got.dtype == np.uint8 and got.tobytes() == u8.tobytes() and np.array_equal(u8, ref.samples(f32))
    jpg, _ = base.processed((("format", "jpeg"), ("quality", 85), ("restart_mcus", 16)))
    assert jpg.tobytes() == utils_image.encode_jpeg(torch.tensor(f32).cuda(), quality=85, restart_mcus=16).tobytes()
    dflt, _ = base.processed((("format", "jpeg"), ("dtype", "uint8")))
    assert dflt.tobytes() == utils_image.encode_jpeg(torch.tensor(f32).cuda()).tobytes()


@pytest.mark.parametrize("output", [{"format": "png", "dtype": "float32"}, {"format": "png", "filter": "paeth2"},
                                    {"format": "png", "interval_bytes": 0}, {"format": "png", "interval_bytes": (1 << 20) + 1},
                                    {"format": "png", "dtype": "int16"}, {"format": "PNG"}])
def test_process_refuses_contradictions(output):
    with pytest.raises(ValueError):
        hsr.process(dict(base.burst()), base.config(output))


def test_command_line_writes_the_returned_bytes(tmp_path):
    spec = importlib.util.spec_from_file_location(
        "hhsr_run_handheld", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                          "handheld-multi-frame-super-resolution_amd", "run_handheld.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    npz = tmp_path / "burst.npz"
    np.savez(npz, **base.burst())
    overrides = ["verbose=0", "scale=2", "block_matching.tuning.tile_size=16", "block_matching.tuning.factors=[1, 2, 2, 2]",
                 "block_matching.tuning.metrics=[L2, L2, L2, L2]", "robustness.save_mask=false", "output.format=png"]
    out = tmp_path / "result.png"
    assert cli.main(["--impath", str(npz), "--outpath", str(out), *overrides]) == 0
    want, _ = base.processed((("format", "png"),))
    assert out.read_bytes() == want.tobytes()
