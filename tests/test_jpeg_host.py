"""JPEG output without a GPU: the header of hhsr_jpeg_header against the restatement tests/jpeg_ref.py byte for byte, the
restated tables and the restated encoder's files against Pillow (libjpeg), every argument refusal of the four entry points
and the worst case hhsr_jpeg_workspace states.  Only host-only entry points are ever called with valid arguments here."""
import ctypes
import functools
import io

import numpy as np
import pytest

import jpeg_ref as ref

from handheld_super_resolution import _lib, utils_image

QUALITIES = [1, 50, 75, 100]
P, SZ = ctypes.c_void_p, ctypes.c_size_t

# Pillow's decode against ref.decode of the same coefficients, measured on the images below on the CPU (maximum over all
# of them): 2 levels for RGB files, 1 for grey ones.  libjpeg's integer IDCT is within 1 level per Y / Cb / Cr sample and its
# colour conversion amplifies that; the bound asserted is measured + 1.
B_RGB, B_GREY = 2 + 1, 1 + 1


# ---- header and tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("components", [1, 3])
@pytest.mark.parametrize("quality", QUALITIES)
def test_header_matches_restatement(quality, components):
    for (H, W), ri in (((40, 72), 65535), ((40, 72), 45), ((40, 72), 44), ((40, 72), 1), ((1, 1), 1), ((65535, 65535), 65535),
                       ((9, 17), 3)):
        want = ref.header(H, W, components, quality, ri)
        got = utils_image.jpeg_header(H, W, components, quality, ri)
        assert got.dtype == np.uint8 and got.tobytes() == want, (H, W, ri)
        dri = b"\xFF\xDD\x00\x04" in want
        assert dri == (ri < ((H + 7) // 8) * ((W + 7) // 8))  # 45 MCUs: Ri = 45 writes no DRI, 44 does
        assert len(want) == {1: 328, 3: 623}[components] + 6 * dri


def test_header_reports_its_length_when_the_buffer_is_short():
    lib = _lib.load()
    buf, n = (ctypes.c_uint8 * 700)(*([0xA5] * 700)), SZ(0)
    assert lib.hhsr_jpeg_header(16, 16, 3, 90, 1, buf, 100, ctypes.byref(n)) == -1 and n.value == 629
    assert all(v == 0xA5 for v in buf)
    assert lib.hhsr_jpeg_header(16, 16, 3, 90, 1, buf, 629, ctypes.byref(n)) == 0 and n.value == 629
    assert bytes(buf[:4]) == b"\xFF\xD8\xFF\xE0" and all(v == 0xA5 for v in buf[629:])


def _pillow_tables(Image, quality):
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=quality, subsampling=0)
    return ref.parse_tables(b.getvalue())


@pytest.mark.parametrize("quality", QUALITIES + [90])
def test_tables_equal_pillows(quality):
    Image = pytest.importorskip("PIL.Image")
    t = _pillow_tables(Image, quality)
    luma, chroma = ref.quant_tables(quality)
    assert t["dqt"][0] == [int(v) for v in luma[ref.ZIGZAG]] and t["dqt"][1] == [int(v) for v in chroma[ref.ZIGZAG]]
    for tcth, (bits, vals) in ref.HUFF_SPECS:  # libjpeg writes K.3 - K.6 when it does not optimise
        assert t["dht"][tcth] == (bits, vals), hex(tcth)
    ours = ref.parse_tables(utils_image.jpeg_header(16, 16, 3, quality, 2).tobytes() + b"\xFF\xDA")
    assert ours["dqt"] == t["dqt"] and ours["dht"] == t["dht"] and ours["dri"] == 2


# ---- the restated encoder's files -----------------------------------------------------------------------------------------------
FILE_SHAPES = [(1, 1), (8, 8), (9, 17), (3, 64), (40, 72), (136, 264)]


@functools.lru_cache(maxsize=None)
def restated(shape, channels, name, quality):
    img = ref.test_images(shape[0], shape[1], channels, seed=shape[0] * 7 + shape[1] + channels)[name]
    coef = ref.coefficients(img, quality)
    coef.setflags(write=False)
    return coef


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", FILE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_restated_file_opens_in_pillow(shape, channels):
    Image = pytest.importorskip("PIL.Image")
    H, W = shape
    worst = 0
    for name in ("random", "smooth", "constant", "wild"):
        for quality, ri in ((50, 1), (90, 4), (100, 65535)):
            coef = restated(shape, channels, name, quality)
            im = Image.open(io.BytesIO(ref.file_bytes(coef, H, W, quality, ri)))
            im.load()
            assert im.size == (W, H) and im.mode == ("L" if channels == 1 else "RGB")
            d = np.abs(np.asarray(im).astype(int) - ref.decode(coef, H, W, quality).astype(int)).max()
            worst = max(worst, int(d))
    print(f"Pillow vs restated decode, {channels} channel(s), {H}x{W}: max {worst}")
    assert worst <= (B_GREY if channels == 1 else B_RGB)


def test_restated_scan_structure():
    """45 MCUs at Ri = 4: 12 intervals, RST0 .. RST7, RST0 .. RST2, no marker after the last; every other 0xFF is stuffed."""
    coef = restated((40, 72), 3, "random", 100)
    scan = ref.scan_bytes(coef, 4)
    i, markers = 0, []
    while i < len(scan):
        if scan[i] == 0xFF:
            assert i + 1 < len(scan)
            if scan[i + 1] != 0:
                markers.append(scan[i + 1])
            i += 2
        else:
            i += 1
    assert markers == [0xD0 + k % 8 for k in range(11)]
    assert len(ref.scan_bytes(coef, 45)) == len(ref.scan_bytes(coef, 65535)) and b"\xFF\xD0" not in ref.scan_bytes(coef, 45)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_do_not_touch_the_gpu():
    """Every refusal include/hhsr.h lists for the four entry points: -1 and "invalid argument" before any HIP call.  The
    pointers are arbitrary aligned addresses — a refused call never uses them."""
    lib = _lib.load()
    H, W, A = 40, 72, 1 << 32
    coef_bytes, scratch_bytes, _ = utils_image.jpeg_workspace(H, W, 3, 4)
    assert coef_bytes == 45 * 3 * 128 and scratch_bytes >= 12 * 12 and scratch_bytes % 4 == 0
    buf, n = (ctypes.c_uint8 * 1024)(), SZ(0)
    a, b, c = SZ(0), SZ(0), SZ(0)
    img, coef, scratch, scan, length = A, A + (1 << 24), A + (2 << 24), A + (3 << 24), A + (4 << 24)
    cap = 1 << 20

    def header(H=H, W=W, ch=3, q=90, ri=4, out=buf, cap=1024, n=ctypes.byref(n)):
        return lib.hhsr_jpeg_header(H, W, ch, q, ri, out, cap, n)

    def workspace(H=H, W=W, ch=3, ri=4, a=ctypes.byref(a), b=ctypes.byref(b), c=ctypes.byref(c)):
        return lib.hhsr_jpeg_workspace(H, W, ch, ri, a, b, c)

    def dct(img=img, H=H, W=W, ch=3, och=3, q=90, coef=coef, nbytes=coef_bytes):
        return lib.hhsr_jpeg_dct(P(img), H, W, ch, och, q, P(coef), nbytes, None)

    def entropy(coef=coef, H=H, W=W, och=3, ri=4, scratch=scratch, sbytes=scratch_bytes, scan=scan, cap=cap, length=length):
        return lib.hhsr_jpeg_entropy(P(coef), H, W, och, ri, P(scratch), sbytes, P(scan), cap, P(length), None)

    sizes = [dict(H=0), dict(W=0), dict(H=-8), dict(H=65536), dict(W=65536)]
    restarts = [dict(ri=0), dict(ri=-1), dict(ri=65536)]
    qualities = [dict(q=0), dict(q=101), dict(q=-5)]
    cases = {
        header: sizes + restarts + qualities + [dict(ch=0), dict(ch=2), dict(ch=4), dict(out=None), dict(n=None),
                                                dict(cap=0), dict(cap=628)],
        workspace: sizes + restarts + [dict(ch=2), dict(a=None), dict(b=None), dict(c=None)],
        dct: sizes + qualities + [
            dict(img=None), dict(coef=None), dict(ch=2), dict(ch=4), dict(ch=1, och=3), dict(och=2), dict(och=0),
            dict(img=img + 2), dict(coef=coef + 8), dict(coef=coef + 2),               # misaligned
            dict(nbytes=coef_bytes - 1), dict(nbytes=0),                               # workspace too small
            dict(coef=img), dict(coef=img + H * W * 12 - 16), dict(img=coef + coef_bytes - 4)],  # overlap
        entropy: sizes + restarts + [
            dict(coef=None), dict(scratch=None), dict(scan=None), dict(length=None), dict(och=2), dict(och=0),
            dict(coef=coef + 8), dict(scratch=scratch + 4), dict(length=length + 4),   # misaligned
            dict(sbytes=scratch_bytes - 1), dict(sbytes=0),                            # workspace too small
            dict(scan=coef), dict(scan=coef + coef_bytes - 1), dict(scan=scratch + 8), dict(scratch=coef),
            dict(length=coef + 16), dict(length=scratch + 8), dict(length=scan + 8), dict(length=scan + cap - 8),
            dict(scan=length - cap + 1)],                                              # overlap, each pair
    }
    missed = []
    for call, bad in cases.items():
        for kw in bad:
            rc = call(**kw)
            if not (rc == -1 and b"invalid argument" in lib.hhsr_last_error()):
                missed.append((call.__name__, kw, rc, lib.hhsr_last_error()))
    assert not missed, missed
    assert header() == 0 and workspace() == 0  # the host-only calls with everything valid
    with pytest.raises(RuntimeError, match="GPU"):
        utils_image.encode_jpeg(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        utils_image.save_jpeg(np.zeros((4, 4), np.uint8), "unused.jpg")


# ---- worst case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("components", [1, 3])
def test_max_scan_bytes_covers_the_worst_coefficients(components):
    """Arrays made to be long: every AC value +-1023 (the longest code of size 10, 16 + 10 bits), the DC alternating between the
    ends of its range (category 11), and values whose codes are runs of 1-bits, so that stuffing doubles bytes."""
    H, W = 16, 24
    n = 6
    rng = np.random.default_rng(3)
    worst = np.full((n, components, 64), -1023, np.int16)
    worst[:, :, 1::2] = 1023
    worst[0::2, :, 0], worst[1::2, :, 0] = -1024, 1023
    wild = rng.integers(-32768, 32768, (n, components, 64)).astype(np.int16)  # clamped on read
    ones = np.zeros((n, components, 64), np.int16)
    ones[:, :, 1:] = -1  # magnitude bits 0 ... the codes' bits dominate; kept as a third pattern
    for ri in (1, 4, 65535):
        _, _, bound = utils_image.jpeg_workspace(H, W, components, ri)
        assert bound == ref.max_scan_bytes(H, W, components, ri)
        for arr in (worst, wild, ones):
            assert len(ref.scan_bytes(arr, ri)) <= bound
    assert len(ref.scan_bytes(worst, 65535)) > 200 * n * components  # the array does come near 216 bytes per block
