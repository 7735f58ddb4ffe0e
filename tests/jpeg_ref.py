"""The JPEG contract of include/hhsr.h ("JPEG output") restated in NumPy and plain Python: what tests/test_jpeg_host.py and
tests/test_jpeg_encode.py compare the library with.  Baseline sequential DCT (ITU-T T.81), JFIF 1.02, 8 bits, 4:4:4.

  samples   q = rint(clip(nan_to_num(x), 0, 1) * 255) in float32, half to even (the 8-bit rule of hhsr_encode_image);
            `components` 1 of a 3-channel image takes channel 0
  colour    Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,
            Cr = 0.5 R - 0.418688 G - 0.081312 B  (T.871 full range; the +128 of Cb / Cr and the level shift cancel); a grey
            file's component is q - 128; nothing is rounded before the transform
  edges     the last column and the last row are replicated up to the next multiple of 8
  DCT       T.81 A.3.3, float64 here; coefficient = rint(c / Q[k]), DC clamped to [-1024, 1023], AC to [-1023, 1023]
  tables    K.1 / K.2 scaled by the IJG rule, K.3 - K.6 as they stand
  scan      one interleaved scan, MCU = one block of each component, restart intervals of `restart_mcus` MCUs
  file      header || scan || FF D9

Coefficient arrays are int16 [n_mcu][components][64] in zig-zag order, MCUs in raster order, DC raw (not differenced)."""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])  # ZIGZAG[k]: row-major index u * 8 + v of the k-th coefficient

K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K2_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# K.3 - K.6: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
    0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
    0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
    0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])
HUFF_SPECS = [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)]  # (Tc << 4 | Th, table), file order


def quant_table(base, quality):
    """IJG scaling of a base table (row-major): s = 5000 // q below 50, else 200 - 2 q; clamp((base s + 50) // 100, 1, 255)."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def quant_tables(quality):
    return quant_table(K1_LUMA, quality), quant_table(K2_CHROMA, quality)


def huff_codes(spec):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table, T.81 annex C."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def mcu_grid(H, W):
    return (H + 7) // 8, (W + 7) // 8


def header(H, W, components, quality, restart_mcus):
    """SOI, APP0 (JFIF 1.02, no units, 1:1, no thumbnail), one DQT segment per table, SOF0, one DHT segment per table (DC
    luma, AC luma[, DC chroma, AC chroma]), DRI when restart_mcus < the number of MCUs, SOS."""
    assert components in (1, 3) and 1 <= restart_mcus <= 65535
    out = b"\xFF\xD8" + b"\xFF\xE0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 2, 0, 1, 1, 0, 0)
    for t, q in enumerate(quant_tables(quality)[: 1 if components == 1 else 2]):
        out += b"\xFF\xDB" + struct.pack(">HB", 67, t) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xFF\xC0" + struct.pack(">HBHHB", 8 + 3 * components, 8, H, W, components)
    for c in range(components):
        out += bytes([c + 1, 0x11, 0 if c == 0 else 1])
    for tcth, (bits, vals) in HUFF_SPECS[: 2 if components == 1 else 4]:
        out += b"\xFF\xC4" + struct.pack(">HB", 19 + len(vals), tcth) + bytes(bits) + bytes(vals)
    my, mx = mcu_grid(H, W)
    if restart_mcus < my * mx:
        out += b"\xFF\xDD" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xFF\xDA" + struct.pack(">HB", 6 + 2 * components, components)
    for c in range(components):
        out += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + bytes([0, 63, 0])


def samples(img, components=None):
    """float image [H, W] or [H, W, 3] -> uint8 samples [H, W, components] by the 8-bit rule (float32, one multiply)."""
    a = np.asarray(img, np.float32)
    a = a[..., None] if a.ndim == 2 else a
    if components == 1:
        a = a[..., :1]
    with np.errstate(invalid="ignore"):
        a = np.clip(np.where(np.isnan(a), np.float32(0), a), np.float32(0), np.float32(1))
    return np.rint(a * np.float32(255)).astype(np.uint8)


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] /= np.sqrt(2.0)
    return m  # m @ f: the 1-D DCT-II of A.3.3


def planes(u8):
    """uint8 samples [H, W, C] -> float64 component planes [C, H, W], level-shifted."""
    s = u8.astype(np.float64)
    if s.shape[2] == 1:
        return s.transpose(2, 0, 1) - 128.0
    r, g, b = s[..., 0], s[..., 1], s[..., 2]
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b - 128.0, -0.168736 * r - 0.331264 * g + 0.5 * b,
                     0.5 * r - 0.418688 * g - 0.081312 * b])


def dct_unquantised(u8):
    """uint8 samples [H, W, C] -> float64 DCT coefficients [n_mcu, C, 64] in zig-zag order, before the division."""
    H, W, C = u8.shape
    my, mx = mcu_grid(H, W)
    p = np.pad(planes(u8), ((0, 0), (0, my * 8 - H), (0, mx * 8 - W)), mode="edge")
    blocks = p.reshape(C, my, 8, mx, 8).transpose(1, 3, 0, 2, 4)  # [my, mx, C, 8, 8]
    m = dct_matrix()
    co = np.einsum("uy,abcyx,vx->abcuv", m, blocks, m).reshape(my * mx, C, 64)
    return co[..., ZIGZAG]


def q_zigzag(components, quality):
    """The divisors [components, 64] in zig-zag order."""
    ql, qc = quant_tables(quality)
    return np.stack([ql[ZIGZAG]] + [qc[ZIGZAG]] * (components - 1)).astype(np.float64)


def quantise(co, quality):
    """float64 coefficients [n, C, 64] -> (int16 coefficients, distance of each to its nearest rounding boundary in
    coefficient units)."""
    Q = q_zigzag(co.shape[1], quality)
    r = co / Q
    q = np.rint(r)
    lo = np.full(64, -1023.0)
    lo[0] = -1024.0
    tie = np.abs(np.abs(r - np.floor(r)) - 0.5) * Q  # | c - (n + 1/2) Q |
    return np.clip(q, lo, 1023.0).astype(np.int16), tie


def coefficients(img, quality, components=None):
    return quantise(dct_unquantised(samples(img, components)), quality)[0]


def _magnitude(v):
    """(category, extra bits) of a DC difference or an AC value."""
    a = abs(v)
    cat = a.bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def clamp_coefficients(coef):
    c = np.asarray(coef).astype(np.int64)
    lo = np.full(64, -1023)
    lo[0] = -1024
    return np.clip(c, lo, 1023)


def ac_strings(coef):
    """The AC part of every block's bit string, [n_mcu][C] of (bits as an integer, their number).  It does not depend on the
    restart interval: scan_bytes takes it back through `ac=` when one array is coded with several."""
    coef = clamp_coefficients(coef)
    n_mcu, C, _ = coef.shape
    tabs = [huff_codes(AC_LUMA)] + [huff_codes(AC_CHROMA)] * (C - 1)
    out = []
    for m in range(n_mcu):
        row = []
        for c in range(C):
            ac = tabs[c]
            acc, nbits, run = 0, 0, 0
            for v in coef[m, c, 1:].tolist():
                if v == 0:
                    run += 1
                    continue
                while run >= 16:  # ZRL
                    code, ln = ac[0xF0]
                    acc, nbits = (acc << ln) | code, nbits + ln
                    run -= 16
                cat, extra = _magnitude(v)
                code, ln = ac[(run << 4) | cat]
                acc, nbits = (((acc << ln) | code) << cat) | extra, nbits + ln + cat
                run = 0
            if run:  # EOB
                code, ln = ac[0x00]
                acc, nbits = (acc << ln) | code, nbits + ln
            row.append((acc, nbits))
        out.append(row)
    return out


def scan_bytes(coef, restart_mcus, ac=None):
    """int coefficients [n_mcu, C, 64] (clamped on read, as the library does) -> the entropy-coded scan: intervals of
    restart_mcus MCUs, each padded with 1-bits, 0xFF stuffed, RSTm between them."""
    coef = clamp_coefficients(coef)
    n_mcu, C, _ = coef.shape
    dc = [huff_codes(DC_LUMA)] + [huff_codes(DC_CHROMA)] * (C - 1)
    ac = ac_strings(coef) if ac is None else ac
    dcs = coef[:, :, 0].tolist()
    out = bytearray()
    n_int = -(-n_mcu // restart_mcus)
    for it in range(n_int):
        acc, nbits = 0, 0
        pred = [0] * C  # the prediction restarts with the interval
        for m in range(it * restart_mcus, min((it + 1) * restart_mcus, n_mcu)):
            for c in range(C):
                cat, extra = _magnitude(dcs[m][c] - pred[c])
                pred[c] = dcs[m][c]
                code, ln = dc[c][cat]
                acc, nbits = (((acc << ln) | code) << cat) | extra, nbits + ln + cat
                abits, an = ac[m][c]
                acc, nbits = (acc << an) | abits, nbits + an
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        out += acc.to_bytes(nbits // 8, "big").replace(b"\xFF", b"\xFF\x00")
        if it + 1 < n_int:
            out += bytes([0xFF, 0xD0 + it % 8])
    return bytes(out)


def file_bytes(coef, H, W, quality, restart_mcus):
    coef = np.asarray(coef)
    return header(H, W, coef.shape[1], quality, restart_mcus) + scan_bytes(coef, restart_mcus) + b"\xFF\xD9"


def encode(img, quality, restart_mcus, components=None):
    """The whole restated encoder: float image -> file bytes."""
    u8 = samples(img, components)
    return file_bytes(quantise(dct_unquantised(u8), quality)[0], u8.shape[0], u8.shape[1], quality, restart_mcus)


def decode(coef, H, W, quality):
    """float64 decoder of a coefficient array: dequantise, IDCT, + 128 and limit to [0, 255], colour, round, clip -> uint8 [H, W] or [H, W, 3]."""
    coef = clamp_coefficients(coef)
    n, C, _ = coef.shape
    my, mx = mcu_grid(H, W)
    nat = np.empty((n, C, 64))
    nat[..., ZIGZAG] = coef * q_zigzag(C, quality)
    m = dct_matrix()
    blocks = np.einsum("uy,abcuv,vx->abcyx", m, nat.reshape(my, mx, C, 8, 8), m)
    p = blocks.transpose(2, 0, 3, 1, 4).reshape(C, my * 8, mx * 8)[:, :H, :W]
    p = np.clip(p + 128.0, 0.0, 255.0)  # a decoded component sample is an 8-bit value: where the quantisation error of a
    if C == 1:                          # noisy block overshoots, every decoder limits Y, Cb and Cr before the colour step
        rgb = p[0]
    else:
        y, cb, cr = p[0], p[1] - 128.0, p[2] - 128.0
        rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def max_scan_bytes(H, W, components, restart_mcus):
    """The bound hhsr_jpeg_workspace states: 27 bits per coefficient (a 16-bit code and 11 magnitude bits) = 216 bytes per
    block, every byte stuffed, 2 bytes per RSTm."""
    my, mx = mcu_grid(H, W)
    n = my * mx
    return 432 * n * components + 2 * (-(-n // restart_mcus) - 1)


def parse_tables(data):
    """{'dqt': {id: [64 zig-zag]}, 'dht': {tcth: (bits, vals)}, 'dri': Ri or None} of a JPEG file's header segments."""
    out, i = {"dqt": {}, "dht": {}, "dri": None}, 2
    while data[i + 1] != 0xDA:
        marker, ln = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + ln]
        if marker == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                out["dqt"][seg[0] & 15] = list(seg[1:65])
                seg = seg[65:]
        elif marker == 0xC4:
            while seg:
                bits = list(seg[1:17])
                out["dht"][seg[0]] = (bits, list(seg[17:17 + sum(bits)]))
                seg = seg[17 + sum(bits):]
        elif marker == 0xDD:
            out["dri"] = struct.unpack(">H", seg)[0]
        i += 2 + ln
    return out


def test_images(H, W, channels, seed):
    """The four kinds of test images, float32 [H, W] or [H, W, 3]: random, smooth plus noise, constant, and one with NaN,
    +-inf and out-of-range samples."""
    rng = np.random.default_rng(seed)
    shape = (H, W) if channels == 1 else (H, W, channels)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    smooth = 0.5 + 0.35 * np.sin(5 * xx + 2 * yy) * np.cos(3 * yy - xx)
    smooth = smooth if channels == 1 else np.stack([smooth, 0.8 * smooth + 0.1 * xx, 1 - smooth * yy], axis=-1)
    wild = rng.uniform(-0.25, 1.25, shape)
    wild.flat[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, 2.0, -1.0, 0.5, 1.0]), wild.flat[::7].size)
    return {"random": rng.uniform(0, 1, shape).astype(np.float32),
            "smooth": (smooth + rng.normal(0, 0.01, shape)).astype(np.float32),
            "constant": np.full(shape, 0.6, np.float32),
            "wild": wild.astype(np.float32)}
