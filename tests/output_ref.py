"""NumPy restatement of the integer output (include/hhsr.h "integer output"): the quantisation of the finished image and
the robustness mask.  Test infrastructure: the yardstick of tests/test_output_*.py.

quantize() is the reference's own arithmetic (run_handheld.py:133-134, then skimage's img_as_ubyte, or
utils_dng.py:212-215 for 16 bits) on float32 input.  mask() is NOT: upstream replicates the map to three channels and
resizes it with OpenCV's INTER_NEAREST, and OpenCV is not available to this project.  The integer index rule below is the
contract; it is OpenCV's rule for integer ratios.  It has never been compared with a real cv2 run (PARITY.md says so)."""
import functools
import struct
import zlib

import numpy as np

F32 = np.float32
LEVELS = {8: 255, 16: 65535}
DTYPES = {8: np.uint8, 16: np.uint16}


def quantize(img, bits):
    """float32 -> uint8 (bits 8) / uint16 (bits 16):  v = nan_to_num(img) (NaN -> 0, +-inf -> +-FLT_MAX);
    v = clip(v, 0, 1);  p = v * float32(M), one float32 multiply rounded once, M = 255 / 65535;  q = rint(p), half to even,
    clipped to [0, M] and cast.  8 bits: skimage.img_as_ubyte of a float32 image (rint(x * 255) after the reference's
    nan_to_num and clip, run_handheld.py:133-134, 151).  16 bits: utils_dng.py:212-215 (x * 65535, np.round, clip,
    astype(uint16))."""
    M = LEVELS[bits]
    v = np.nan_to_num(np.asarray(img, dtype=F32))
    v = np.clip(v, F32(0), F32(1))
    p = v * F32(M)
    assert p.dtype == F32
    return np.clip(np.rint(p), 0, M).astype(DTYPES[bits])


def mask(acc, n_comp, out_shape):
    """Oriented accumulated robustness float32 [ah, aw] -> grey uint8 [mH, mW] (run_handheld.py:153-159, one channel):
    a = acc / float32(n_comp);  out[y, x] = quantize(a[min((y ah) // mH, ah - 1), min((x aw) // mW, aw - 1)], 8)."""
    acc = np.asarray(acc, dtype=F32)
    ah, aw = acc.shape
    mH, mW = (int(v) for v in out_shape)
    a = acc / F32(n_comp)
    assert a.dtype == F32
    iy = np.minimum((np.arange(mH, dtype=np.int64) * ah) // mH, ah - 1)
    ix = np.minimum((np.arange(mW, dtype=np.int64) * aw) // mW, aw - 1)
    return quantize(a[iy][:, ix], 8)


@functools.lru_cache(maxsize=None)
def _samples(bits):
    M = LEVELS[bits]
    ties = ((np.arange(M, dtype=np.float64) + 0.5) / M).astype(F32)  # float32((k + 0.5) / M), k = 0 .. M - 1
    one = F32(1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1e-3, -5.0, -3e38, 1.0 + 1e-3, 2.0, 3e38, 1.0,
                        np.nextafter(one, F32(0)), 1e-40, np.finfo(F32).tiny, 0.5], dtype=F32)
    out = np.concatenate([special, ties])  # (the special values first: the smallest test images hold them)
    out.setflags(write=False)
    return out


def samples(bits):
    """The fixture (read-only float32 vector): NaN, +-inf, -0.0, 0, negatives, values above 1, 1.0, nextafter(1, 0), a
    denormal, FLT_MIN and 0.5, then every float32((k + 0.5) / M) — all M of them land exactly on k + 0.5 after the float32
    multiply, the ties of rint, and for the even k half-to-even differs from half-up (tests/test_output_host.py asserts
    both counts)."""
    return _samples(bits)


def make_image(shape, channels, bits, seed):
    """float32 [H, W] (channels 1) or [H, W, 3]: the samples fixture tiled over the image; behind its first copy, which
    stays whole, a seeded half of the samples is replaced by noise in [-0.2, 1.3]."""
    H, W = shape
    n = H * W * channels
    s = samples(bits)
    v = np.resize(s, n).astype(F32)
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-0.2, 1.3, n).astype(F32)
    pick = rng.random(n) < 0.5
    pick[:s.size] = False
    v[pick] = noise[pick]
    return v.reshape((H, W) if channels == 1 else (H, W, channels))


# ---- the written files, read back with struct and zlib alone --------------------------------------------------------------
def parse_png(path):
    """(IHDR fields, pixel array) of a PNG whose rows all have filter type 0; every chunk's CRC is checked."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and len(chunks[0][1]) == 13
    assert all(t == b"IDAT" for t, _ in chunks[1:-1]) and len(chunks) >= 3
    W, H, depth, colour, comp, flt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, flt, interlace) == (0, 0, 0) and depth in (8, 16) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks[1:-1])), np.uint8)
    stride = W * ch * depth // 8 + 1
    assert raw.size == H * stride
    rows = raw.reshape(H, stride)
    assert not rows[:, 0].any()  # filter type 0 on every row
    px = np.ascontiguousarray(rows[:, 1:])
    px = px.view(">u2").astype(np.uint16) if depth == 16 else px  # 16-bit samples are big-endian
    return (W, H, depth, colour), px.reshape((H, W, 3) if ch == 3 else (H, W))


def parse_tiff(path):
    """({tag: (type, count, values)}, pixel array) of a little-endian baseline TIFF with one uncompressed strip."""
    data = open(path, "rb").read()
    order, magic, ifd = struct.unpack("<2sHI", data[:8])
    assert order == b"II" and magic == 42
    (n,) = struct.unpack("<H", data[ifd:ifd + 2])
    size = {3: 2, 4: 4, 5: 8}
    tags, last = {}, 0
    for i in range(n):
        e = data[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
        tag, typ, count = struct.unpack("<HHI", e[:8])
        assert tag > last, "IFD entries ascend"
        last = tag
        nbytes = size[typ] * count
        src = e[8:8 + nbytes] if nbytes <= 4 else data[struct.unpack("<I", e[8:])[0]:][:nbytes]
        tags[tag] = (typ, count, struct.unpack("<%d%s" % (count * (2 if typ == 5 else 1), {3: "H", 4: "I", 5: "I"}[typ]), src))
    assert struct.unpack("<I", data[ifd + 2 + 12 * n:ifd + 6 + 12 * n])[0] == 0  # a single IFD
    W, H, spp = tags[256][2][0], tags[257][2][0], tags[277][2][0]
    bits = tags[258][2]
    assert len(bits) == spp and len(set(bits)) == 1 and bits[0] in (8, 16)
    assert tags[259][2] == (1,) and tags[284][2] == (1,)          # uncompressed, chunky
    assert tags[262][2] == ((2,) if spp == 3 else (1,))           # RGB / BlackIsZero
    assert tags[278][2] == (H,) and tags[273][1] == 1             # one strip
    off, nbytes = tags[273][2][0], tags[279][2][0]
    assert nbytes == H * W * spp * bits[0] // 8 and off + nbytes == len(data) and off % 2 == 0
    px = np.frombuffer(data[off:off + nbytes], "<u2" if bits[0] == 16 else np.uint8)
    return tags, px.reshape((H, W, 3) if spp == 3 else (H, W))
