"""Lossless JPEG (ITU-T T.81 Annex H, SOF3, Huffman) restated with NumPy and the standard library: an encoder and a decoder
for any precision P 2..16, Nf 1..4 interleaved components and predictors 1..7, Huffman tables built per stream by the
procedure of Annex K.2 or one fixed table that uses 16-bit codes.  The tests' reference for hhsr_ljpeg_*; the encoder is
pinned by an independent decoder in tests/test_ljpeg_host.py."""
import numpy as np

# One fixed table with 16-bit codes: one code each of 2..15 bits, three of 16 bits (Kraft sum < 1); SSSS 0..16 in order,
# so SSSS 14, 15 and 16 take the 16-bit codes
FIXED_BITS = [0] + [1] * 14 + [3]
FIXED_VALUES = list(range(17))


def predictions(s, P, predictor):
    """Annex H predictions of the samples s [Y, X, Nf] (int64): 2^(P-1) for the first sample, Ra on the first line, Rb in the
    first column, else the predictor's rule."""
    s = np.asarray(s, np.int64)
    Ra = np.zeros_like(s)
    Rb = np.zeros_like(s)
    Rc = np.zeros_like(s)
    Ra[:, 1:] = s[:, :-1]
    Rb[1:] = s[:-1]
    Rc[1:, 1:] = s[:-1, :-1]
    p = {1: Ra, 2: Rb, 3: Rc, 4: Ra + Rb - Rc, 5: Ra + ((Rb - Rc) >> 1), 6: Rb + ((Ra - Rc) >> 1), 7: (Ra + Rb) >> 1}[predictor]
    p = p.copy()
    p[0, 1:] = Ra[0, 1:]
    p[1:, 0] = Rb[1:, 0]
    p[0, 0] = 1 << (P - 1)
    return p


def categories(s, P, predictor):
    """(difference in -32767..32768, SSSS) per sample, modulo 2^16."""
    d = (np.asarray(s, np.int64) - predictions(s, P, predictor)) & 0xFFFF
    d = np.where(d > 32768, d - 65536, d)
    ssss = np.searchsorted(2 ** np.arange(16, dtype=np.int64), np.abs(d), side="right")
    return d, ssss


def build_k2(freq):
    """(bits[16], values) by Annex K.2 from the 17 SSSS frequencies."""
    freq = [int(f) for f in freq]
    assert len(freq) == 17 and sum(freq) > 0
    f = freq + [1]  # the reserved code point
    n = len(f)
    codesize, others = [0] * n, [-1] * n
    while True:  # Figure K.1
        live = [i for i in range(n) if f[i] > 0]
        if len(live) < 2:
            break
        v1 = max((i for i in live if f[i] == min(f[j] for j in live)))
        rest = [i for i in live if i != v1]
        v2 = max((i for i in rest if f[i] == min(f[j] for j in rest)))
        f[v1] += f[v2]
        f[v2] = 0
        codesize[v1] += 1
        while others[v1] >= 0:
            v1 = others[v1]
            codesize[v1] += 1
        others[v1] = v2
        codesize[v2] += 1
        while others[v2] >= 0:
            v2 = others[v2]
            codesize[v2] += 1
    bits = [0] * 33
    for i in range(n):
        if codesize[i]:
            bits[codesize[i]] += 1
    i = 32  # Figure K.3
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
    bits[i] -= 1  # the reserved code point leaves
    values = [v for size in range(1, 33) for v in range(17) if codesize[v] == size]  # Figure K.4
    return bits[1:17], values


def codes_of(bits, values):
    """{SSSS: (code, length)} of a DHT (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def entropy_bits(d, ssss, tables, comp_table):
    """The scan's bit string as a uint8 array of 0 / 1: per sample (line by line, components interleaved) the Huffman code
    of SSSS, then the SSSS low bits of d (d - 1 when negative); nothing behind SSSS 0 and 16."""
    Y, X, Nf = d.shape
    code = np.zeros((Y, X, Nf), np.uint64)
    clen = np.zeros((Y, X, Nf), np.int64)
    for c in range(Nf):
        cod = codes_of(*tables[comp_table[c]])
        lut_c = np.zeros(17, np.uint64)
        lut_l = np.zeros(17, np.int64)
        for sv, (cc, ll) in cod.items():
            lut_c[sv], lut_l[sv] = cc, ll
        assert (lut_l[ssss[:, :, c]] > 0).all(), "a category without a code"
        code[:, :, c] = lut_c[ssss[:, :, c]]
        clen[:, :, c] = lut_l[ssss[:, :, c]]
    nx = np.where(ssss == 16, 0, ssss)
    extra = np.where(d < 0, d + (1 << nx) - 1, d) & ((1 << nx) - 1)
    val = ((code << nx.astype(np.uint64)) | extra.astype(np.uint64)).reshape(-1)
    L = (clen + nx).reshape(-1)
    j = np.arange(32, dtype=np.int64)
    shift = L[:, None] - 1 - j[None, :]
    mask = shift >= 0
    bits = ((val[:, None] >> np.maximum(shift, 0).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return bits[mask]


def encode(samples, P, predictor=1, tables="k2", comp_table=None, restart=None):
    """samples [Y, X, Nf] (or [Y, X]) -> the stream's bytes: SOI, SOF3, DHT, SOS, entropy-coded data, EOI.
    tables: "k2" (one table per component, built from that component's categories), "k2shared" (one for all), "fixed"
    (FIXED_BITS / FIXED_VALUES), or a list of (bits, values) with comp_table naming one per component."""
    s = np.asarray(samples, np.int64)
    if s.ndim == 2:
        s = s[:, :, None]
    Y, X, Nf = s.shape
    assert 2 <= P <= 16 and 1 <= Nf <= 4 and 1 <= predictor <= 7 and s.min() >= 0 and s.max() < (1 << P)
    d, ssss = categories(s, P, predictor)
    if tables == "k2":
        tables = [build_k2(np.bincount(ssss[:, :, c].reshape(-1), minlength=17)) for c in range(Nf)]
        comp_table = list(range(Nf))
    elif tables == "k2shared":
        tables, comp_table = [build_k2(np.bincount(ssss.reshape(-1), minlength=17))], [0] * Nf
    elif tables == "fixed":
        tables, comp_table = [(FIXED_BITS, FIXED_VALUES)], [0] * Nf
    bits = entropy_bits(d, ssss, tables, comp_table)
    pad = (-bits.size) % 8
    data = np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)])).tobytes().replace(b"\xff", b"\xff\x00")
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xc3" + (8 + 3 * Nf).to_bytes(2, "big") + bytes([P]) + Y.to_bytes(2, "big") + X.to_bytes(2, "big") + bytes([Nf])
    for c in range(Nf):
        out += bytes([c + 1, 0x11, 0])
    for i, (b, v) in enumerate(tables):
        out += b"\xff\xc4" + (2 + 1 + 16 + len(v)).to_bytes(2, "big") + bytes([i]) + bytes(b) + bytes(v)
    if restart is not None:
        out += b"\xff\xdd\x00\x04" + int(restart).to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * Nf).to_bytes(2, "big") + bytes([Nf])
    for c in range(Nf):
        out += bytes([c + 1, comp_table[c] << 4])
    out += bytes([predictor, 0, 0])
    return bytes(out + data + b"\xff\xd9")


def split(stream):
    """(header fields, entropy-coded bytes) of a stream this module wrote: {"P", "Y", "X", "Nf", "predictor", "tables":
    {id: (bits, values)}, "comp_table", "data_offset"}."""
    assert stream[:2] == b"\xff\xd8"
    p, h = 2, {"tables": {}}
    while True:
        assert stream[p] == 0xFF
        m, n = stream[p + 1], int.from_bytes(stream[p + 2:p + 4], "big")
        b = stream[p + 4:p + 2 + n]
        if m == 0xC3:
            h.update(P=b[0], Y=int.from_bytes(b[1:3], "big"), X=int.from_bytes(b[3:5], "big"), Nf=b[5])
        elif m == 0xC4:
            q = 0
            while q < len(b):
                bits = list(b[q + 1:q + 17])
                h["tables"][b[q] & 15] = (bits, list(b[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xDA:
            nf = b[0]
            h["comp_table"] = [b[2 + 2 * c] >> 4 for c in range(nf)]
            h["predictor"] = b[1 + 2 * nf]
            p += 2 + n
            break
        p += 2 + n
    h["data_offset"] = p
    end = stream.rfind(b"\xff\xd9")
    return h, stream[p:end if end >= p else len(stream)]


def decode(stream):
    """The samples [Y, X, Nf] (int64) of a stream: bit by bit, in plain Python."""
    h, data = split(stream)
    data = data.replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(data, np.uint8)).tolist()
    P, Y, X, Nf, pred = h["P"], h["Y"], h["X"], h["Nf"], h["predictor"]
    inv = []
    for c in range(Nf):
        inv.append({(code, length): sv for sv, (code, length) in codes_of(*h["tables"][h["comp_table"][c]]).items()})
    s = np.zeros((Y, X, Nf), np.int64)
    at = 0
    for y in range(Y):
        for x in range(X):
            for c in range(Nf):
                code, length = 0, 0
                while True:
                    code, length, at = (code << 1) | bits[at], length + 1, at + 1
                    if (code, length) in inv[c]:
                        break
                    assert length < 16, "no code"
                sv = inv[c][(code, length)]
                if sv == 0:
                    d = 0
                elif sv == 16:
                    d = 32768
                else:
                    v = 0
                    for _ in range(sv):
                        v, at = (v << 1) | bits[at], at + 1
                    d = v if v >= (1 << (sv - 1)) else v - (1 << sv) + 1
                if y == 0:
                    p = (1 << (P - 1)) if x == 0 else s[0, x - 1, c]
                elif x == 0:
                    p = s[y - 1, 0, c]
                else:
                    Ra, Rb, Rc = int(s[y, x - 1, c]), int(s[y - 1, x, c]), int(s[y - 1, x - 1, c])
                    p = [Ra, Rb, Rc, Ra + Rb - Rc, Ra + ((Rb - Rc) >> 1), Rb + ((Ra - Rc) >> 1), (Ra + Rb) >> 1][pred - 1]
                s[y, x, c] = (int(p) + d) & 0xFFFF
    return s


def to_stream_geometry(rect, Nf, X):
    """A segment's rectangle of counts [h, w] as the samples [Y, X, Nf] of a stream: the flat row-major order of the
    rectangle cut into lines of X Nf samples (h w a multiple of X Nf)."""
    rect = np.asarray(rect)
    assert rect.size % (X * Nf) == 0
    return rect.reshape(-1, X, Nf)
