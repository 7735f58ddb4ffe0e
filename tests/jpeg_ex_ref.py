"""The extended JPEG contract of include/hhsr.h ("JPEG output, extended") restated in NumPy and plain Python, on top of
tests/jpeg_ref.py: 4:2:0 chroma subsampling and Huffman tables made for the image.

  4:2:0     MCU = 16 x 16 pixels, edges replicated up to the next multiple of 16; Y as in 4:4:4; a Cb / Cr sample is the
            unrounded mean of its 2 x 2 pixels; blocks Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr; SOF0 factors 0x22 / 0x11 / 0x11;
            the DC prediction runs per component in coding order and restarts with the interval of 16 x 16 MCUs
  tables    a specification is (BITS[1..16], HUFFVAL) as in jpeg_ref; `specs` lists DC luma, AC luma[, DC chroma, AC chroma];
            as an array: uint8 [n][16 + 256], zero-filled
  counts    counts[t][s]: how often the scan emits symbol s of table t
  K.2       libjpeg's jpeg_gen_optimal_table, see huffman()

Coefficient arrays are int16 [n_mcu][blocks per MCU][64]; `sub` is 0 (4:4:4) or 1 (4:2:0)."""
import struct

import numpy as np

import jpeg_ref as ref

STANDARD = [ref.DC_LUMA, ref.AC_LUMA, ref.DC_CHROMA, ref.AC_CHROMA]


def mcu_grid(H, W, sub=0):
    s = 16 if sub else 8
    return (H + s - 1) // s, (W + s - 1) // s


def components_of(blocks_per_mcu, sub=0):
    """The component of every block position of an MCU."""
    return [0, 0, 0, 0, 1, 2] if sub else list(range(blocks_per_mcu))


def workspace(H, W, components, restart_mcus, sub=0):
    """(coef_bytes, the entropy coder's scratch bytes, the histogram's scratch bytes, max_scan_bytes)."""
    my, mx = mcu_grid(H, W, sub)
    n = my * mx
    bpm = 6 if sub else components
    n_int = -(-n // restart_mcus)
    entropy = (n_int + -(-n_int // 2048)) * 8 + n_int * 4
    hist = min(-(-n * bpm // 256), 512) * 8192
    return 128 * n * bpm, entropy, hist, 432 * n * bpm + 2 * (n_int - 1)


def spec_array(specs):
    out = np.zeros((len(specs), 272), np.uint8)
    for t, (bits, vals) in enumerate(specs):
        out[t, :16] = bits
        out[t, 16:16 + len(vals)] = vals
    return out


def header(H, W, components, quality, restart_mcus, sub=0, specs=None):
    """jpeg_ref.header with the sampling factors of `sub` and the DHT segments of `specs` (None: K.3 - K.6)."""
    assert components in (1, 3) and 1 <= restart_mcus <= 65535 and (not sub or components == 3)
    specs = STANDARD[:2 if components == 1 else 4] if specs is None else specs
    assert len(specs) == (2 if components == 1 else 4)
    out = b"\xFF\xD8" + b"\xFF\xE0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 2, 0, 1, 1, 0, 0)
    for t, q in enumerate(ref.quant_tables(quality)[: 1 if components == 1 else 2]):
        out += b"\xFF\xDB" + struct.pack(">HB", 67, t) + bytes(int(v) for v in q[ref.ZIGZAG])
    out += b"\xFF\xC0" + struct.pack(">HBHHB", 8 + 3 * components, 8, H, W, components)
    for c in range(components):
        out += bytes([c + 1, 0x22 if (sub and c == 0) else 0x11, 0 if c == 0 else 1])
    for tcth, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), specs):
        out += b"\xFF\xC4" + struct.pack(">HB", 19 + len(vals), tcth) + bytes(bits) + bytes(vals)
    my, mx = mcu_grid(H, W, sub)
    if restart_mcus < my * mx:
        out += b"\xFF\xDD" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xFF\xDA" + struct.pack(">HB", 6 + 2 * components, components)
    for c in range(components):
        out += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + bytes([0, 63, 0])


# ---- 4:2:0 coefficients -------------------------------------------------------------------------------------------------------
def dct_unquantised_420(u8):
    """uint8 samples [H, W, 3] -> float64 DCT coefficients [n_mcu, 6, 64] in zig-zag order, before the division."""
    H, W, C = u8.shape
    assert C == 3
    my, mx = mcu_grid(H, W, 1)
    p = np.pad(ref.planes(u8), ((0, 0), (0, my * 16 - H), (0, mx * 16 - W)), mode="edge")
    m = ref.dct_matrix()
    y = p[0].reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, 4, 8, 8)  # Y(r, c) at 2 r + c
    ch = 0.25 * ((p[1:, 0::2, 0::2] + p[1:, 0::2, 1::2]) + (p[1:, 1::2, 0::2] + p[1:, 1::2, 1::2]))
    ch = ch.reshape(2, my, 8, mx, 8).transpose(1, 3, 0, 2, 4)
    blocks = np.concatenate([y, ch], axis=2)  # [my, mx, 6, 8, 8]
    co = np.einsum("uy,abcyx,vx->abcuv", m, blocks, m).reshape(my * mx, 6, 64)
    return co[..., ref.ZIGZAG]


def q_zigzag_420(quality):
    ql, qc = ref.quant_tables(quality)
    return np.stack([ql[ref.ZIGZAG]] * 4 + [qc[ref.ZIGZAG]] * 2).astype(np.float64)


def quantise_420(co, quality):
    """jpeg_ref.quantise for [n, 6, 64]: (int16 coefficients, distance to the nearest rounding boundary)."""
    Q = q_zigzag_420(quality)
    r = co / Q
    lo = np.full(64, -1023.0)
    lo[0] = -1024.0
    tie = np.abs(np.abs(r - np.floor(r)) - 0.5) * Q
    return np.clip(np.rint(r), lo, 1023.0).astype(np.int16), tie


def coefficients(img, quality, sub=0, components=None):
    u8 = ref.samples(img, components)
    if not sub:
        return ref.quantise(ref.dct_unquantised(u8), quality)[0]
    return quantise_420(dct_unquantised_420(u8), quality)[0]


def y_of_444(coef444, H, W):
    """The Y blocks of a 4:4:4 array [n, C, 64] of an H x W image, arranged as the 4:2:0 array holds them: [n_mcu16, 4, 64],
    and a mask of the positions that exist in the 4:4:4 grid (a 16 x 16 MCU may reach one block beyond it)."""
    my8, mx8 = ref.mcu_grid(H, W)
    my, mx = mcu_grid(H, W, 1)
    y = np.zeros((my * 2, mx * 2, 64), coef444.dtype)
    have = np.zeros((my * 2, mx * 2), bool)
    y[:my8, :mx8] = coef444[:, 0].reshape(my8, mx8, 64)
    have[:my8, :mx8] = True
    y = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, 4, 64)
    have = have.reshape(my, 2, mx, 2).transpose(0, 2, 1, 3).reshape(my * mx, 4)
    return y, have


# ---- symbols, counts, scan ----------------------------------------------------------------------------------------------------
def block_symbols(coef, restart_mcus, sub=0):
    """Every block's symbols in coding order: [n_mcu][blocks] of (table 0 luma / 1 chroma, [(is_ac, symbol, value, size)])."""
    coef = ref.clamp_coefficients(coef)
    n_mcu, B, _ = coef.shape
    comp = components_of(B, sub)
    out = []
    pred = {}
    for m in range(n_mcu):
        if m % restart_mcus == 0:
            pred = {}
        row = []
        for b in range(B):
            vals = coef[m, b].tolist()
            d = vals[0] - pred.get(comp[b], 0)
            pred[comp[b]] = vals[0]
            syms = [(0, abs(d).bit_length(), d, abs(d).bit_length())]
            run = 0
            for v in vals[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    syms.append((1, 0xF0, 0, 0))
                    run -= 16
                size = abs(v).bit_length()
                syms.append((1, (run << 4) | size, v, size))
                run = 0
            if run:
                syms.append((1, 0x00, 0, 0))
            row.append((0 if comp[b] == 0 else 1, syms))
        out.append(row)
    return out


def histogram(coef, restart_mcus, sub=0, symbols=None):
    """uint64 [4][256]: rows DC luma, AC luma, DC chroma, AC chroma."""
    counts = np.zeros((4, 256), np.uint64)
    for row in block_symbols(coef, restart_mcus, sub) if symbols is None else symbols:
        for tab, syms in row:
            for is_ac, s, _, _ in syms:
                counts[2 * tab + is_ac, s] += np.uint64(1)
    return counts


def scan_bytes(coef, restart_mcus, sub=0, specs=None, symbols=None):
    """The entropy-coded scan with the tables of `specs` (None: K.3 - K.6), or None if a symbol has no code."""
    n_mcu = np.asarray(coef).shape[0]
    specs = STANDARD if specs is None else specs
    codes = [ref.huff_codes(s) for s in specs]
    symbols = block_symbols(coef, restart_mcus, sub) if symbols is None else symbols
    out = bytearray()
    n_int = -(-n_mcu // restart_mcus)
    for it in range(n_int):
        acc, nbits = 0, 0
        for m in range(it * restart_mcus, min((it + 1) * restart_mcus, n_mcu)):
            for tab, syms in symbols[m]:
                for is_ac, s, v, size in syms:
                    if s not in codes[2 * tab + is_ac]:
                        return None
                    code, ln = codes[2 * tab + is_ac][s]
                    extra = (v if v >= 0 else v - 1) & ((1 << size) - 1)
                    acc, nbits = (((acc << ln) | code) << size) | extra, nbits + ln + size
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        out += acc.to_bytes(nbits // 8, "big").replace(b"\xFF", b"\xFF\x00")
        if it + 1 < n_int:
            out += bytes([0xFF, 0xD0 + it % 8])
    return bytes(out)


# ---- K.2 ------------------------------------------------------------------------------------------------------------------------
def code_lengths(counts):
    """T.81 K.2 / Figure K.1 as libjpeg runs it: {symbol: length before any limiting}, the reserved symbol 256 included.
    The two least non-zero counts are merged; each search keeps the LAST of equal counts (the larger symbol index)."""
    freq = [int(c) for c in counts] + [1]
    assert len(freq) == 257
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        v = None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return {s: n for s, n in enumerate(codesize) if n}


def huffman(counts):
    """counts[256] -> (BITS, HUFFVAL), or None when every count is zero: K.2, lengths above 16 shortened by Figure K.3, the
    reserved symbol removed from the longest length in use, HUFFVAL ordered by (length found by K.2, symbol)."""
    if not any(int(c) for c in counts):
        return None
    size = code_lengths(counts)
    top = max(size.values())
    bits = [0] * (max(top, 16) + 1)
    for n in size.values():
        bits[n] += 1
    i = len(bits) - 1
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for n, s in sorted((n, s) for s, n in size.items() if s != 256)]
    return bits[1:17], vals


def huffman_specs(counts, components):
    return [huffman(counts[t]) for t in range(2 if components == 1 else 4)]


# ---- files ------------------------------------------------------------------------------------------------------------------------
def file_bytes(coef, H, W, quality, restart_mcus, sub=0, specs=None, components=None):
    coef = np.asarray(coef)
    components = (3 if sub else coef.shape[1]) if components is None else components
    scan = scan_bytes(coef, restart_mcus, sub, specs)
    return header(H, W, components, quality, restart_mcus, sub, specs) + scan + b"\xFF\xD9"


def _upsample_fancy(c):
    """libjpeg's h2v2 "fancy" upsampling of an integer plane, edges replicated: 3 near + far vertically, then
    (3 this + neighbour + 8 or 7) >> 4 horizontally."""
    c = c.astype(np.int64)
    up, down = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    rows = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    rows[0::2], rows[1::2] = 3 * c + up, 3 * c + down
    left, right = np.hstack([rows[:, :1], rows[:, :-1]]), np.hstack([rows[:, 1:], rows[:, -1:]])
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return out


def decode_420(coef, H, W, quality):
    """float64 decoder of a 4:2:0 array: dequantise, IDCT, + 128, Y / Cb / Cr ROUNDED to 8 bits, the chroma planes of
    ceil(H / 2) x ceil(W / 2) samples upsampled as libjpeg does, colour, round, clip -> uint8 [H, W, 3]."""
    coef = ref.clamp_coefficients(coef)
    my, mx = mcu_grid(H, W, 1)
    nat = np.empty((coef.shape[0], 6, 64))
    nat[..., ref.ZIGZAG] = coef * q_zigzag_420(quality)
    m = ref.dct_matrix()
    blocks = np.einsum("uy,abcuv,vx->abcyx", m, nat.reshape(my, mx, 6, 8, 8), m)
    blocks = np.clip(np.rint(blocks + 128.0), 0, 255)
    y = blocks[:, :, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)[:H, :W]
    ch = blocks[:, :, 4:].transpose(2, 0, 3, 1, 4).reshape(2, my * 8, mx * 8)[:, :(H + 1) // 2, :(W + 1) // 2]
    cb, cr = (_upsample_fancy(p)[:H, :W] - 128.0 for p in ch)
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def sof_factors(data):
    """[(component id, sampling factors byte, quantisation table)] of a file's SOF0."""
    data = bytes(data)
    i = data.index(b"\xFF\xC0")
    n = data[i + 9]
    return [tuple(data[i + 10 + 3 * c:i + 13 + 3 * c]) for c in range(n)]
