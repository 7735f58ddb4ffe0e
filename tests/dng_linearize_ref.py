"""The NumPy restatement of include/hhsr.h, "DNG linearization" (hhsr_linearize_raw_u16), operation by operation in
float32 with the map coordinates in float64, and a writer of OpcodeList2 (51009) whose bytes go through
dng_ref.write_dng(extra=[opcode_list_entry(...)]).  An opcode list is big-endian whatever the file's byte order."""
import struct

import numpy as np

import dng_ref

F32 = np.float32
OPCODE_LIST2 = 51009
UNDEFINED = 7


def axis(n, origin, spacing, points):
    """(i0, i1, fraction float32) per pixel of an axis of n pixels: step 3 of the contract."""
    i0, i1, f = np.zeros(n, np.intp), np.zeros(n, np.intp), np.zeros(n, F32)
    if points == 1:
        return i0, i1, f
    for p in range(n):
        u = ((np.float64(p) + np.float64(0.5)) / np.float64(n) - np.float64(origin)) / np.float64(spacing)
        if u <= 0:
            continue
        if u >= points - 1:
            i0[p] = i1[p] = points - 1
            continue
        r = np.floor(u)
        i0[p], i1[p], f[p] = int(r), int(r) + 1, F32(u - r)
    return i0, i1, f


def gain_plane(m, H, W):
    """g of every pixel of an H x W image under the map m (a dict: gains [PV, PH], origin_v / _h, spacing_v / _h)."""
    g = np.asarray(m["gains"], F32)
    r0, r1, fv = axis(H, m["origin_v"], m["spacing_v"], g.shape[0])
    c0, c1, fh = axis(W, m["origin_h"], m["spacing_h"], g.shape[1])
    one = F32(1)
    fv, fh = fv[:, None], fh[None, :]
    R0, R1, C0, C1 = r0[:, None], r1[:, None], c0[None, :], c1[None, :]
    t0 = g[R0, C0] * (one - fv) + g[R1, C0] * fv
    t1 = g[R0, C1] * (one - fv) + g[R1, C1] * fv
    out = t0 * (one - fh) + t1 * fh
    assert out.dtype == F32
    return out


def covered(m, H, W):
    """Boolean [H, W]: the pixels the map applies to (pitch 1: all; pitch 2: one position of the 2 x 2 cell)."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    if m["row_pitch"] == 1:
        return np.ones((H, W), bool)
    return (y % 2 == m["top"]) & (x % 2 == m["left"])


def linearize(counts, black, white, wb, cfa, table=None, delta_h=None, delta_v=None, maps=()):
    """counts [n, H, W] (integers) -> float32 [n, H, W]: steps 1 - 4."""
    counts = np.asarray(counts).astype(np.int64)
    n, H, W = counts.shape
    lin = np.asarray(table, np.uint16)[np.minimum(counts, len(table) - 1)] if table is not None else counts
    lin = lin.astype(F32)
    colour = np.asarray(cfa)[np.arange(H)[:, None] & 1, np.arange(W)[None, :] & 1]
    dh = np.zeros(W, F32) if delta_h is None else np.asarray(delta_h, F32)
    dv = np.zeros(H, F32) if delta_v is None else np.asarray(delta_v, F32)
    b = (np.array([F32(v) for v in black[:3]], F32)[colour] + dh[None, :]) + dv[:, None]
    den = F32(white) - b
    v = (lin - b[None]) / den[None]
    for m in maps:
        mask = covered(m, H, W)
        g = gain_plane(m, H, W)
        v[:, mask] = v[:, mask] * g[mask][None]
    gain = np.array([F32(wb[c] / wb[1]) for c in range(3)], F32)[colour]
    v = v * gain[None]
    assert v.dtype == F32
    return v


def make_map(gains, origin=(0.0, 0.0), spacing=(1.0, 1.0), top=0, left=0, pitch=2, bottom=1 << 16, right=1 << 16):
    g = np.asarray(gains, F32)
    return dict(gains=g, origin_v=float(origin[0]), origin_h=float(origin[1]), spacing_v=float(spacing[0]),
                spacing_h=float(spacing[1]), top=top, left=left, row_pitch=pitch, col_pitch=pitch, bottom=bottom, right=right,
                points_v=g.shape[0], points_h=g.shape[1])


# ---- OpcodeList2 ------------------------------------------------------------------------------------------------------------
def opcode(opcode_id, params, flags=0, version=(1, 3, 0, 0), size=None):
    return struct.pack(">I4BII", opcode_id, *version, flags, len(params) if size is None else size) + params


def gain_map_opcode(m, plane=0, planes=1, map_planes=1, points=None, flags=0, size=None, row_pitch=None, col_pitch=None):
    """Opcode 9 of the map dict m; the keywords override single fields for the refusal tests."""
    g = np.asarray(m["gains"], F32)
    pv, ph = points if points is not None else g.shape
    params = struct.pack(">10I4dI", m["top"], m["left"], m["bottom"], m["right"], plane, planes,
                         m["row_pitch"] if row_pitch is None else row_pitch, m["col_pitch"] if col_pitch is None else col_pitch,
                         pv, ph, m["spacing_v"], m["spacing_h"], m["origin_v"], m["origin_h"], map_planes)
    return opcode(9, params + g.astype(">f4").tobytes(), flags, size=size)


def opcode_list(opcodes, count=None):
    return struct.pack(">I", len(opcodes) if count is None else count) + b"".join(opcodes)


def opcode_list_entry(opcodes, count=None, cut=None):
    """The (tag, BYTE, values) entry for dng_ref.write_dng(extra=...); `cut`: only that many bytes of the list."""
    data = opcode_list(opcodes, count)
    return (OPCODE_LIST2, dng_ref.BYTE, list(data if cut is None else data[:cut]))


def retype_undefined(path, byte_order):
    """dng_ref writes field type BYTE: patch the entry of tag 51009 in the file at `path` to UNDEFINED (7).  The IFDs lie
    behind the data blocks, so the last occurrence of (tag, BYTE) is the entry."""
    e = "<" if byte_order == "II" else ">"
    data = bytearray(open(path, "rb").read())
    at = bytes(data).rfind(struct.pack(e + "HH", OPCODE_LIST2, dng_ref.BYTE))
    assert at > 0
    struct.pack_into(e + "H", data, at + 2, UNDEFINED)
    with open(path, "wb") as f:
        f.write(bytes(data))
