"""NumPy / Python restatement of the "PNG output" contract of include/hhsr.h: samples, filters and the adaptive choice, byte
counts, canonical codes, the interval coder (it takes `spec` — code lengths and block header — from the library or from
anywhere else), file assembly with zlib.crc32 / zlib.adler32, the cost of the optimal length-limited code by
package-merge, and a decoder (parse + unfilter) for the files Pillow does not keep exactly."""
import struct
import zlib

import numpy as np

FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
SPEC_BYTES = 768
SPEC_BITS_AT, SPEC_HDR_AT = 258, 260


# ---- 1. samples -------------------------------------------------------------------------------------------------------------
def samples(img, bits=8, channels=None):
    """float32 [H, W] or [H, W, 3] -> uint8 / uint16 of hhsr_encode_image's rule; channels=1: channel 0."""
    a = np.asarray(img, np.float32)
    if channels == 1 and a.ndim == 3:
        a = a[..., 0]
    M = np.float32(255 if bits == 8 else 65535)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(a), np.float32(0), a)
        x = np.minimum(np.maximum(x, np.float32(0)), np.float32(1))
        return np.rint(x * M).astype(np.uint8 if bits == 8 else np.uint16)


def row_bytes(q):
    """integer samples [H, W] or [H, W, 3] -> (uint8 [H, W * bpp], bpp): 16-bit samples big-endian."""
    H = q.shape[0]
    och = 1 if q.ndim == 2 else q.shape[2]
    rows = np.ascontiguousarray(q.astype(">u2") if q.dtype == np.uint16 else q).reshape(H, -1).view(np.uint8)
    return rows, och * q.dtype.itemsize


# ---- 2. filters ---------------------------------------------------------------------------------------------------------------
def candidates(rows, bpp):
    """uint8 [H, R] -> int [5, H, R]: every row under None, Sub, Up, Average, Paeth (PNG 9.2, 9.4)."""
    x = rows.astype(np.int32)
    H, R = x.shape
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :R - bpp] if R > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :R - bpp] if R > bpp else 0
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255])


def filtered_stream(rows, bpp, filt):
    """(the filtered stream uint8 [H * (1 + R)], the filter type of every row); filt 0 .. 4, or 5: libpng's heuristic."""
    cand = candidates(rows, bpp)
    H, R = rows.shape
    if filt == 5:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # [5, H]
        types = np.argmin(cost, axis=0)                            # (the first minimum: ties to the lowest type)
    else:
        types = np.full(H, filt)
    out = np.empty((H, 1 + R), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out.reshape(-1), types


def unfilter(stream, H, R, bpp):
    """The inverse: filtered stream -> uint8 [H, R]."""
    s = np.asarray(stream, np.uint8).reshape(H, 1 + R)
    out = np.zeros((H, R), np.int32)
    for y in range(H):
        t, f = int(s[y, 0]), s[y, 1:].astype(np.int32)
        up = out[y - 1] if y else np.zeros(R, np.int32)
        if t == 0:
            out[y] = f
        elif t == 2:
            out[y] = (f + up) & 255
        else:
            row = out[y]
            for i in range(R):
                a = row[i - bpp] if i >= bpp else 0
                b = up[i]
                c = up[i - bpp] if i >= bpp else 0
                if t == 1:
                    p = a
                elif t == 3:
                    p = (a + b) >> 1
                elif t == 4:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                else:
                    raise ValueError(f"filter type {t}")
                row[i] = (f[i] + p) & 255
    return out.astype(np.uint8)


def byte_counts(stream):
    return np.bincount(np.asarray(stream, np.uint8), minlength=256).astype(np.uint64)


def n_intervals(N, interval):
    return -(-N // interval)


# ---- 3. codes -----------------------------------------------------------------------------------------------------------------
def canonical_codes(lens):
    """RFC 1951 3.2.2: code lengths -> code words (MSB-first integers)."""
    lens = [int(v) for v in lens]
    bl = [0] * 17
    for v in lens:
        bl[v] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for v in lens:
        out.append(nxt[v] if v else 0)
        if v:
            nxt[v] += 1
    return out


def package_merge_cost(counts, limit=15):
    """The least sum count x length of a prefix code with lengths <= limit over the symbols of non-zero count
    (package-merge, Larmore & Hirschberg): the cost is the weight of the first 2 m - 2 items of the top level."""
    w = sorted(int(c) for c in counts if int(c))
    m = len(w)
    assert 2 <= m <= 1 << limit
    level = list(w)
    for _ in range(limit - 1):
        packages = [level[i] + level[i + 1] for i in range(0, len(level) - 1, 2)]
        level = sorted(w + packages)
    return sum(level[:2 * m - 2])


def spec_parts(spec):
    """spec -> (code lengths [257], header bit count, header bits as a list of 0 / 1)."""
    s = np.asarray(spec, np.uint8)
    assert s.shape == (SPEC_BYTES,)
    nbits = int(s[SPEC_BITS_AT]) | int(s[SPEC_BITS_AT + 1]) << 8
    hdr = np.unpackbits(s[SPEC_HDR_AT:], bitorder="little")[:nbits]
    return s[:257].astype(int), nbits, hdr.astype(np.uint8)


# ---- 4. the interval coder ------------------------------------------------------------------------------------------------------
def coder(spec):
    """spec -> block(piece, last): the bytes of one interval — its dynamic-Huffman block (header with BFINAL = last, one code
    per byte, the end code), then 000 and the empty stored block's 00 00 FF FF unless it is the last, zero-padded to bytes."""
    lens, nbits, hdr = spec_parts(spec)
    codes = canonical_codes(lens)
    # every symbol's code as bits in stream order: MSB of the code first
    sym_bits = [np.array([(codes[s] >> (lens[s] - 1 - k)) & 1 for k in range(lens[s])], np.uint8) for s in range(257)]

    def block(piece, last):
        assert all(lens[int(v)] > 0 for v in np.unique(piece)), "a byte value without a code"
        parts = [hdr.copy()]
        parts[0][0] = 1 if last else 0
        parts += [sym_bits[int(v)] for v in piece]
        parts.append(sym_bits[256])
        if not last:
            parts.append(np.zeros(3, np.uint8))
        bits = np.concatenate(parts)
        bits = np.concatenate([bits, np.zeros(-bits.size % 8, np.uint8)])
        return np.packbits(bits, bitorder="little").tobytes() + (b"" if last else b"\x00\x00\xff\xff")

    return block


def deflate(stream, interval, spec):
    """The deflate stream of include/hhsr.h "intervals": interval k covers stream[k I, min((k + 1) I, N))."""
    data = np.asarray(stream, np.uint8)
    block = coder(spec)
    n_int = n_intervals(data.size, interval)
    if interval == 1:  # (the same bytes, quickly: a one-byte interval that is not the last is one of 256 strings)
        table = {int(v): block(np.array([v], np.uint8), False) for v in np.unique(data[:-1])}
        return b"".join([table[int(v)] for v in data[:-1]]) + block(data[-1:], True)
    return b"".join(block(data[k * interval:(k + 1) * interval], k + 1 == n_int) for k in range(n_int))


# ---- 5. the file ----------------------------------------------------------------------------------------------------------------
def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def file_head(H, W, och, bits, deflate_len):
    ihdr = struct.pack(">IIBBBBB", W, H, bits, 2 if och == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + struct.pack(">I", deflate_len + 6) + b"IDAT\x78\x01"


def file_tail(deflate_bytes, stream):
    adler = struct.pack(">I", zlib.adler32(bytes(stream)) & 0xFFFFFFFF)
    crc = zlib.crc32(b"IDAT\x78\x01" + deflate_bytes + adler) & 0xFFFFFFFF
    return adler + struct.pack(">I", crc) + chunk(b"IEND", b"")


def png_file(H, W, och, bits, stream, interval, spec):
    d = deflate(stream, interval, spec)
    return file_head(H, W, och, bits, len(d)) + d + file_tail(d, np.asarray(stream, np.uint8).tobytes())


def parse(file_bytes):
    """A file of this module's layout -> (H, W, och, bits, the zlib payload of its one IDAT chunk)."""
    b = bytes(file_bytes)
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, ihdr = 8, [], None
    while at < len(b):
        (n,), tag = struct.unpack(">I", b[at:at + 4]), b[at + 4:at + 8]
        body = b[at + 8:at + 8 + n]
        assert struct.unpack(">I", b[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        at += 12 + n
    assert tag == b"IEND" and at == len(b) and len(idat) == 1
    W, H, bits, ctype, comp, flt, lace = ihdr
    assert (comp, flt, lace) == (0, 0, 0) and ctype in (0, 2)
    return H, W, 3 if ctype == 2 else 1, bits, idat[0]


def decode(file_bytes):
    """A file -> its integer samples, [H, W] or [H, W, 3], uint8 or uint16 (zlib inflates, this module unfilters)."""
    H, W, och, bits, payload = parse(file_bytes)
    bpp = och * bits // 8
    rows = unfilter(np.frombuffer(zlib.decompress(payload), np.uint8), H, W * bpp, bpp)
    q = rows.view(">u2").astype(np.uint16) if bits == 16 else rows
    return q.reshape((H, W) if och == 1 else (H, W, och))


# ---- CRC-32 of a concatenation, as polynomial arithmetic on Python integers ----------------------------------------------------------
_P = (1 << 32) | 0x04C11DB7  # x^32 + x^26 + ... + 1; bit k of an integer: the coefficient of x^k


def _rev32(v):
    return int(f"{v & 0xFFFFFFFF:032b}"[::-1], 2)


def _mulmod(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 32:
            a ^= _P
    return r


def crc_combine(crc_a, crc_b, len_b):
    """crc32(A || B) = crc32(A) x^(8 len B) mod P + crc32(B): the register is the bit-reversed polynomial, and the
    pre- and post-conditioning of the two CRCs cancel."""
    x, e, n = 1, 2, 8 * int(len_b)  # x^n by squaring
    while n:
        if n & 1:
            x = _mulmod(x, e)
        e = _mulmod(e, e)
        n >>= 1
    return _rev32(_mulmod(_rev32(crc_a), x)) ^ (crc_b & 0xFFFFFFFF)


# ---- test images ------------------------------------------------------------------------------------------------------------------
def test_images(H, W, channels, seed):
    """The four kinds of tests/jpeg_ref.py, float32 [H, W] or [H, W, 3]: random, smooth plus noise, constant, and one with
    NaN, +-inf and out-of-range samples."""
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


def five_filter_image(W, channels, seed=3):
    """float32 [10, W(, 3)] of exact 8-bit levels: two rows built to favour each filter type under libpng's heuristic — None
    (values near 0 and near 255 at random: small as signed bytes, every prediction off by ~255 half of the time), Sub
    (horizontal ramps under unrelated rows), Up (noise, then its copy), Average ((left + up) / 2 up to +-1, on top of
    noise), Paeth (rows that follow the Paeth predictor of the rows above).  Which type wins a row also depends on its
    neighbours, so the callers ASSERT on filtered_stream() that all five types are chosen; they do not assume it."""
    rng = np.random.default_rng(seed)
    C = channels
    n = W * C
    rows = np.zeros((10, W, C), np.int64)

    def noise():
        return rng.integers(0, 256, (W, C))

    # None: values in {0..3} and {252..255} at random: small as signed bytes, every predictor is off by ~255 half of the time
    for y in (0, 1):
        rows[y] = np.where(rng.integers(0, 2, (W, C)) == 1, rng.integers(0, 4, (W, C)), rng.integers(252, 256, (W, C)))
    # Sub: ramps, above them the None rows (unrelated)
    for y in (2, 3):
        rows[y] = ((np.arange(W)[:, None] * 3 + 40 * y + np.arange(C)[None, :] * 50) % 256)
    # Up: noise, then its copy
    rows[4] = noise()
    rows[5] = rows[4]
    # Average: on top of row 5 (noise)
    for y in (6, 7):
        for x in range(W):
            left = rows[y, x - 1] if x else np.zeros(C, np.int64)
            rows[y, x] = ((left + rows[y - 1, x]) >> 1) + rng.integers(-1, 2, C)
        rows[y] &= 255
    # Paeth: the row above is piecewise constant with jumps; this row = a step pattern that follows left, except at the jumps
    base = (np.arange(W) // 5 * 37 % 256)
    for y in (8, 9):
        up = rows[y - 1]
        for x in range(W):
            left = rows[y, x - 1] if x else np.zeros(C, np.int64)
            ul = up[x - 1] if x else np.zeros(C, np.int64)
            p = left + up[x] - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up[x]), np.abs(p - ul)
            rows[y, x] = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up[x], ul)) + (base[x] % 2 == 0) * rng.integers(-1, 2, C)
        rows[y] &= 255
    img = (rows.astype(np.float64) / 255.0).astype(np.float32)
    assert n == img[0].size
    return img[..., 0] if C == 1 else img
