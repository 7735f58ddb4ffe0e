"""DNG bursts without rawpy / exifread: the TIFF container read with `struct` (parse_dng), the raw frames brought to the
GPU in the form the file holds them (read_dng_burst) — lossless-JPEG tiles and strips (Compression 7) decoded by
hhsr_ljpeg_decode, uncompressed 16-bit counts, or packed 10/12/14-bit rows — and normalised there.  Opt-in:
``config.dng = {"reader": "native"}`` (super_resolution.load_burst).  Every offset and count of a file is checked against
its size before it is used; what the reader does not handle is a ValueError that names the tag.  PARITY.md, "DNG input",
lists what this was never compared with: no file of a camera or of Adobe's converter, no rawpy / LibRaw decode.
``config.dng.linearization: apply`` (parse_dng / read_dng_burst with linearization=True) reads LinearizationTable,
BlackLevelDeltaH / V and the GainMap opcodes of OpcodeList2 instead of refusing or ignoring them, and
utils_dng.linearize_burst applies them on the GPU (PARITY.md, "DNG linearization")."""
import ctypes
import glob
import os
import struct
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .utils_dng import linearize_burst, normalize_burst, normalize_packed, packed_row_bytes, unpack_raw

MAX_IFD_ENTRIES = 512
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
_TYPE_FMT = {1: "B", 2: "B", 3: "H", 4: "I", 6: "b", 7: "B", 8: "h", 9: "i", 11: "f", 12: "d", 13: "I"}
TAGS = {254: "NewSubFileType", 256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression",
        262: "PhotometricInterpretation", 266: "FillOrder", 273: "StripOffsets", 274: "Orientation", 277: "SamplesPerPixel",
        278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration", 322: "TileWidth", 323: "TileLength",
        324: "TileOffsets", 325: "TileByteCounts", 330: "SubIFDs", 33421: "CFARepeatPatternDim", 33422: "CFAPattern",
        34665: "ExifIFD", 34855: "ISOSpeedRatings", 50712: "LinearizationTable", 50713: "BlackLevelRepeatDim",
        50714: "BlackLevel", 50715: "BlackLevelDeltaH", 50716: "BlackLevelDeltaV", 50717: "WhiteLevel",
        50721: "ColorMatrix1", 50728: "AsShotNeutral", 50729: "AsShotWhiteXY", 50761: "NoiseProfile", 50829: "ActiveArea",
        51009: "OpcodeList2"}
_ID = {name: tag for tag, name in TAGS.items()}

# One stream of the raw image: where its bytes are in the file and the rectangle it covers
Segment = namedtuple("Segment", "offset length x0 y0 seg_w seg_h")

DngInfo = namedtuple("DngInfo", "path byte_order width height bits compression layout segments cfa_pattern black_levels "
                                "white_level white_balance orientation xyz2cam noise_profile iso raw_ifd_offset file_size "
                                "linearization_table black_delta_h black_delta_v gain_maps", defaults=(None,) * 4)
DngInfo.__doc__ = """What parse_dng reads from one file.  `layout`: "strips" or "tiles"; `segments`: Segment per strip / tile
in file order; `cfa_pattern`: 2 x 2 list of 0 / 1 / 2; `black_levels`: (R, G, B); `white_balance`: 1 / AsShotNeutral (list of
3) or None; `orientation`, `xyz2cam` (3 x 3 float32), `noise_profile` (list of floats) and `iso` (clamped to 100..3200): None
when the tag is absent.  Only with parse_dng(linearization=True), None otherwise and when the file has none:
`linearization_table` (uint16 ndarray, 1 .. 65536 entries), `black_delta_h` / `black_delta_v` (float32 ndarrays of `width` /
`height` entries; an all-zero tag is None), `gain_maps` (list of GainMap from OpcodeList2)."""

GainMap = namedtuple("GainMap", "top left bottom right plane planes row_pitch col_pitch points_v points_h spacing_v spacing_h "
                                "origin_v origin_h map_planes gains")
GainMap.__doc__ = """One GainMap opcode (ID 9) of OpcodeList2 with the parameter names of the DNG specification; `gains`:
float32 ndarray [points_v, points_h]."""
MAX_GAIN_POINTS = 64  # per axis of a map: what hhsr_linearize_raw_u16 holds of one map row


def _name(tag):
    return f"{TAGS.get(tag, 'tag')} ({tag})"


class _Tiff:
    """Bounded reads of one classic TIFF held in memory."""

    def __init__(self, data, path):
        self.d, self.n, self.path = data, len(data), path
        if self.n < 8:
            raise ValueError(f"{path}: {self.n} bytes are no TIFF header")
        bo = data[:2]
        if bo not in (b"II", b"MM"):
            raise ValueError(f"{path}: byte order {bo!r} is neither II nor MM")
        self.e = "<" if bo == b"II" else ">"
        self.byte_order = bo.decode()
        magic = struct.unpack_from(self.e + "H", data, 2)[0]
        if magic == 43:
            raise ValueError(f"{path}: BigTIFF (magic 43) is not read, classic TIFF only")
        if magic != 42:
            raise ValueError(f"{path}: TIFF magic {magic} instead of 42")
        self.first_ifd = struct.unpack_from(self.e + "I", data, 4)[0]

    def ifd(self, off, what):
        """{tag: (type, count, offset of the value bytes)} of the IFD at `off`, and the offset of the next IFD."""
        if off < 8 or off + 2 > self.n:
            raise ValueError(f"{self.path}: {what} at offset {off} is outside the file ({self.n} bytes)")
        cnt = struct.unpack_from(self.e + "H", self.d, off)[0]
        if cnt > MAX_IFD_ENTRIES:
            raise ValueError(f"{self.path}: {what} at offset {off} has {cnt} entries, more than {MAX_IFD_ENTRIES}")
        if off + 2 + 12 * cnt + 4 > self.n:
            raise ValueError(f"{self.path}: {what} at offset {off} with {cnt} entries ends outside the file")
        out = {}
        for i in range(cnt):
            p = off + 2 + 12 * i
            tag, typ, count = struct.unpack_from(self.e + "HHI", self.d, p)
            size = _TYPE_SIZE.get(typ)
            if size is None:
                continue  # an unknown field type: TIFF says to skip the entry
            nbytes = size * count  # (Python integers: a count that would overflow 32 bits is simply too large below)
            at = p + 8 if nbytes <= 4 else struct.unpack_from(self.e + "I", self.d, p + 8)[0]
            if at + nbytes > self.n:
                raise ValueError(f"{self.path}: {_name(tag)}: {count} values of type {typ} at offset {at} end outside the "
                                 f"file ({self.n} bytes)")
            out.setdefault(tag, (typ, count, at))
        nxt = struct.unpack_from(self.e + "I", self.d, off + 2 + 12 * cnt)[0]
        return out, nxt

    def values(self, ifd, tag, max_count=None):
        """The values of `tag` as a list of int / float (rationals divided), or None when the IFD has no such tag."""
        if tag not in ifd:
            return None
        typ, count, at = ifd[tag]
        if max_count is not None and count > max_count:
            raise ValueError(f"{self.path}: {_name(tag)} has {count} values, at most {max_count} expected")
        if typ in (5, 10):
            raw = struct.unpack_from(self.e + str(2 * count) + ("I" if typ == 5 else "i"), self.d, at)
            if any(d == 0 for d in raw[1::2]):
                raise ValueError(f"{self.path}: {_name(tag)} holds a rational with denominator 0")
            return [n / d for n, d in zip(raw[::2], raw[1::2])]
        return list(struct.unpack_from(self.e + str(count) + _TYPE_FMT[typ], self.d, at))

    def ints(self, ifd, tag, max_count):
        """values() of an integer tag (BYTE, SHORT or LONG)."""
        if tag in ifd and ifd[tag][0] not in (1, 3, 4):
            raise ValueError(f"{self.path}: {_name(tag)} has field type {ifd[tag][0]}, an integer type expected")
        return self.values(ifd, tag, max_count)

    def one(self, ifd, tag, default=None):
        v = self.ints(ifd, tag, 1)
        if v is None or len(v) != 1:
            if v is None and default is not None:
                return default
            raise ValueError(f"{self.path}: {_name(tag)} is missing or has no single value")
        return v[0]


def _segments(t, ifd, W, H):
    """(layout, [Segment]) of the raw IFD, every stream inside the file and the table as long as the image needs."""
    tiled = _ID["TileOffsets"] in ifd or _ID["TileWidth"] in ifd
    if tiled:
        tw, th = t.one(ifd, _ID["TileWidth"]), t.one(ifd, _ID["TileLength"])
        if tw < 1 or th < 1:
            raise ValueError(f"{t.path}: TileWidth (322) / TileLength (323) {tw} x {th}")
        across, down = -(-W // tw), -(-H // th)
        need, otag, ctag = across * down, _ID["TileOffsets"], _ID["TileByteCounts"]
    else:
        rps = min(t.one(ifd, _ID["RowsPerStrip"], default=2 ** 32 - 1), H)
        if rps < 1:
            raise ValueError(f"{t.path}: RowsPerStrip (278) is 0")
        need, otag, ctag = -(-H // rps), _ID["StripOffsets"], _ID["StripByteCounts"]
    offs, cnts = t.ints(ifd, otag, need), t.ints(ifd, ctag, need)
    if offs is None or cnts is None:
        raise ValueError(f"{t.path}: {_name(otag)} / {_name(ctag)} missing")
    if len(offs) != need or len(cnts) != need:
        raise ValueError(f"{t.path}: {_name(otag)} has {len(offs)} and {_name(ctag)} {len(cnts)} entries, the image of "
                         f"{W} x {H} needs {need}")
    segs = []
    for i, (o, c) in enumerate(zip(offs, cnts)):
        if o + c > t.n or c < 1:
            raise ValueError(f"{t.path}: {_name(otag)}[{i}] = {o} with {c} bytes is outside the file ({t.n} bytes)")
        if tiled:
            segs.append(Segment(o, c, (i % across) * tw, (i // across) * th, tw, th))
        else:
            segs.append(Segment(o, c, 0, i * rps, W, min(rps, H - i * rps)))
    return ("tiles" if tiled else "strips"), segs


def _opcode_list2(t, ifd, W, H):
    """The GainMap records of OpcodeList2 (51009), or None without the tag or without a GainMap in it.  The list is
    big-endian whatever the file's byte order: a LONG count, then per opcode OpcodeID, DNG version, flags and the byte size
    of its parameters (LONG each) and the parameters.  Every size is checked against the tag's byte count before it is used.
    Another opcode is skipped when its flag bit 0 (optional) is set and refused by its ID otherwise."""
    tag = _ID["OpcodeList2"]
    if tag not in ifd:
        return None
    typ, nbytes, at = ifd[tag]
    name, path = _name(tag), t.path
    if typ not in (1, 7):
        raise ValueError(f"{path}: {name} has field type {typ}, BYTE or UNDEFINED expected")
    end = at + nbytes

    def need(p, n, what):
        if p + n > end:
            raise ValueError(f"{path}: {name} is truncated: {what} needs {n} bytes at byte {p - at} of {nbytes}")

    need(at, 4, "the opcode count")
    count = struct.unpack_from(">I", t.d, at)[0]
    p, maps, phases = at + 4, [], set()
    for i in range(count):
        need(p, 16, f"the header of opcode {i}")
        oid, _, flags, size = struct.unpack_from(">4I", t.d, p)
        p += 16
        need(p, size, f"the parameters of opcode {i} (OpcodeID {oid})")
        if oid != 9:
            if not flags & 1:
                raise ValueError(f"{path}: {name}: opcode {i} with OpcodeID {oid} is not applied and not marked optional")
            p += size
            continue
        what = f"{path}: {name}: opcode {i} (GainMap)"
        if size < 76:
            raise ValueError(f"{what}: parameter size {size} is below the 76 bytes of its fixed fields")
        top, left, bottom, right, plane, planes, rp, cp, pv, ph = struct.unpack_from(">10I", t.d, p)
        sv, sh, ov, oh = struct.unpack_from(">4d", t.d, p + 40)
        mp = struct.unpack_from(">I", t.d, p + 72)[0]
        for field, v in (("MapPointsV", pv), ("MapPointsH", ph)):
            if not 1 <= v <= MAX_GAIN_POINTS:
                raise ValueError(f"{what}: {field} {v} outside 1 .. {MAX_GAIN_POINTS}")
        if mp != 1:
            raise ValueError(f"{what}: MapPlanes {mp}: one plane per map only")
        if planes != 1 or plane != 0:
            raise ValueError(f"{what}: Plane {plane} / Planes {planes}: plane 0 of a one-plane image only")
        if size != 76 + 4 * pv * ph * mp:
            raise ValueError(f"{what}: parameter size {size} disagrees with MapPointsV x MapPointsH x MapPlanes = "
                             f"{pv} x {ph} x {mp} gains ({76 + 4 * pv * ph * mp} bytes)")
        for field, s, n in (("MapSpacingV", sv, pv), ("MapSpacingH", sh, ph)):
            if n > 1 and not (np.isfinite(s) and s > 0):
                raise ValueError(f"{what}: {field} {s} with {n} points: a positive spacing expected")
        for field, o in (("MapOriginV", ov), ("MapOriginH", oh)):
            if not np.isfinite(o):
                raise ValueError(f"{what}: {field} {o} is not finite")
        gains = np.frombuffer(t.d, ">f4", pv * ph, p + 76).astype(np.float32).reshape(pv, ph)
        if not np.isfinite(gains).all():
            raise ValueError(f"{what}: a non-finite gain")
        if (rp, cp) == (1, 1):
            if (top, left) != (0, 0):
                raise ValueError(f"{what}: Top {top} / Left {left} with RowPitch = ColPitch = 1: 0 / 0 expected")
            cover = {0, 1, 2, 3}
        elif (rp, cp) == (2, 2):
            if top > 1 or left > 1:
                raise ValueError(f"{what}: Top {top} / Left {left} with RowPitch = ColPitch = 2: 0 or 1 expected")
            cover = {top * 2 + left}
        else:
            raise ValueError(f"{what}: RowPitch {rp} / ColPitch {cp}: 1 / 1 (every pixel) or 2 / 2 (one Bayer plane) only")
        if cover & phases:
            raise ValueError(f"{what}: a second map for the pixels at Top {top} / Left {left}, RowPitch {rp} / ColPitch {cp}")
        phases |= cover
        if bottom < H or right < W:
            raise ValueError(f"{what}: Bottom {bottom} / Right {right} do not reach the image's {H} x {W}: a map that "
                             "covers part of the image is not applied")
        maps.append(GainMap(top, left, bottom, right, plane, planes, rp, cp, pv, ph, sv, sh, ov, oh, mp, gains))
        p += size
    return maps or None


def _linearization(t, raw, W, H):
    """(linearization_table, black_delta_h, black_delta_v, gain_maps) of the raw IFD, each None when absent."""
    path = t.path
    tag = _ID["LinearizationTable"]
    table = None
    if tag in raw:
        typ, count, _ = raw[tag]
        if typ != 3:
            raise ValueError(f"{path}: {_name(tag)} has field type {typ}, SHORT expected")
        if not 1 <= count <= 65536:
            raise ValueError(f"{path}: {_name(tag)} has {count} entries, 1 .. 65536 expected")
        table = np.array(t.values(raw, tag), np.uint16)
    deltas = []
    for tag, n, axis in ((_ID["BlackLevelDeltaH"], W, "ImageWidth"), (_ID["BlackLevelDeltaV"], H, "ImageLength")):
        d = None
        if tag in raw:
            if raw[tag][1] != n:
                raise ValueError(f"{path}: {_name(tag)} has {raw[tag][1]} entries, {axis} = {n} expected")
            d = np.array(t.values(raw, tag), np.float32)
            if not np.isfinite(d).all():
                raise ValueError(f"{path}: {_name(tag)} holds a non-finite entry")
            d = d if d.any() else None
        deltas.append(d)
    maps = _opcode_list2(t, raw, W, H)
    tag = _ID["ActiveArea"]
    if tag in raw and (deltas[0] is not None or deltas[1] is not None or maps):
        area = t.ints(raw, tag, 4)
        if area != [0, 0, H, W]:
            raise ValueError(f"{path}: {_name(tag)} {area} is not the whole image [0, 0, {H}, {W}]: the black deltas and the "
                             "gain maps' relative coordinates are defined on the active area, and the full image is read")
    return table, deltas[0], deltas[1], maps


def parse_dng(path, linearization=False):
    """The DngInfo of one .dng file: classic TIFF (II / MM), the raw image in IFD0 or one of its SubIFDs (tag 330, one level):
    the IFD with NewSubFileType 0 and PhotometricInterpretation 32803 (CFA).  Refused by name (ValueError): BigTIFF, LinearRaw
    (34892), Compression other than 1 and 7, SamplesPerPixel != 1, FillOrder != 1, PlanarConfiguration != 1, a CFA that is not
    2 x 2 of R / G / B, BlackLevelRepeatDim other than 1 x 1 and 2 x 2, non-zero BlackLevelDeltaH / V, LinearizationTable,
    AsShotWhiteXY without AsShotNeutral.  ActiveArea, DefaultCrop and the opcode lists are ignored, as the reference ignores
    them (it reads rawpy's full raw_image).  A malformed container — an offset or count outside the file, an IFD loop, a
    strip or tile table shorter than the image needs — is a ValueError naming the tag or offset.

    `linearization=True` reads what is refused or ignored above instead, into the last four fields of the record:
    LinearizationTable (SHORT, 1 .. 65536 entries), BlackLevelDeltaH / V (exactly ImageWidth / ImageLength entries) and the
    GainMap opcodes of OpcodeList2 (_opcode_list2) — one map with RowPitch = ColPitch = 1 at Top = Left = 0, or up to four
    with pitches 2 and Top, Left in {0, 1}, one per position of the 2 x 2 cell at most, each reaching the image's last row
    and column, one plane, 1 .. 64 points per axis.  Anything else about them is a ValueError naming the tag, opcode or
    field; so is an ActiveArea (50829) other than the whole image next to a non-zero delta or a map.  OpcodeList1 and
    OpcodeList3 stay ignored.  utils_dng.linearize_burst applies the four."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        data = f.read()
    t = _Tiff(data, path)
    visited, main = set(), []  # the chain from IFD0
    off = t.first_ifd
    while off:
        if off in visited:
            raise ValueError(f"{path}: the IFD chain returns to offset {off} (a loop)")
        visited.add(off)
        ifd, off = t.ifd(off, "IFD")
        main.append(ifd)
        if len(main) > 64:
            raise ValueError(f"{path}: more than 64 IFDs in the chain")
    if not main:
        raise ValueError(f"{path}: no IFD0")
    ifd0 = main[0]
    cands = [(t.first_ifd, ifd0)]
    for sub in (t.ints(ifd0, _ID["SubIFDs"], 64) or []):
        if sub in visited:
            raise ValueError(f"{path}: SubIFDs (330) points at offset {sub}, an IFD already read (a loop)")
        visited.add(sub)
        cands.append((sub, t.ifd(sub, "SubIFD")[0]))
    raw, raw_off = None, None
    for o, ifd in cands:
        if t.one(ifd, _ID["NewSubFileType"], default=0) != 0 and _ID["NewSubFileType"] in ifd:
            continue
        photo = t.ints(ifd, _ID["PhotometricInterpretation"], 1)
        if photo == [34892]:
            raise ValueError(f"{path}: PhotometricInterpretation (262) 34892 (LinearRaw) is not read, CFA (32803) only")
        if photo == [32803]:
            raw, raw_off = ifd, o
            break
    if raw is None:
        raise ValueError(f"{path}: no IFD with NewSubFileType (254) 0 and PhotometricInterpretation (262) 32803 (CFA)")

    W, H = t.one(raw, _ID["ImageWidth"]), t.one(raw, _ID["ImageLength"])
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"{path}: ImageWidth (256) x ImageLength (257) = {W} x {H} outside 1..65535")
    if t.one(raw, _ID["SamplesPerPixel"], default=1) != 1:
        raise ValueError(f"{path}: SamplesPerPixel (277) other than 1")
    bits = t.one(raw, _ID["BitsPerSample"])
    comp = t.one(raw, _ID["Compression"], default=1)
    if comp not in (1, 7):
        raise ValueError(f"{path}: Compression (259) {comp} is not read: 1 (none) and 7 (lossless JPEG) only")
    if comp == 1 and bits not in (10, 12, 14, 16):
        raise ValueError(f"{path}: BitsPerSample (258) {bits} uncompressed: 10, 12, 14 or 16 only")
    if comp == 7 and not 2 <= bits <= 16:
        raise ValueError(f"{path}: BitsPerSample (258) {bits} with Compression 7: 2..16 only")
    if t.one(raw, _ID["FillOrder"], default=1) != 1:
        raise ValueError(f"{path}: FillOrder (266) other than 1")
    if t.one(raw, _ID["PlanarConfiguration"], default=1) != 1:
        raise ValueError(f"{path}: PlanarConfiguration (284) other than 1")
    layout, segs = _segments(t, raw, W, H)
    if comp == 1 and layout == "tiles" and bits != 16:
        raise ValueError(f"{path}: packed {bits}-bit tiles (TileOffsets (324) with BitsPerSample (258) {bits}) are not read")
    if comp == 1:
        for i, s in enumerate(segs):
            need = s.seg_h * (s.seg_w * 2 if bits == 16 else packed_row_bytes(W, f"be{bits}"))
            if s.length < need:
                raise ValueError(f"{path}: {'TileByteCounts (325)' if layout == 'tiles' else 'StripByteCounts (279)'}[{i}] = "
                                 f"{s.length}, its {s.seg_w} x {s.seg_h} samples need {need} bytes")

    if t.ints(raw, _ID["CFARepeatPatternDim"], 2) != [2, 2]:
        raise ValueError(f"{path}: CFARepeatPatternDim (33421) other than 2 x 2")
    cfa = t.ints(raw, _ID["CFAPattern"], 4)
    if cfa is None or len(cfa) != 4 or sorted(cfa) != [0, 1, 1, 2]:
        raise ValueError(f"{path}: CFAPattern (33422) {cfa}: one red (0), two green (1), one blue (2) expected")
    dim = t.ints(raw, _ID["BlackLevelRepeatDim"], 2) or [1, 1]
    if dim not in ([1, 1], [2, 2]):
        raise ValueError(f"{path}: BlackLevelRepeatDim (50713) {dim}: 1 x 1 or 2 x 2 only")
    bl = t.values(raw, _ID["BlackLevel"], 4) or [0.0] * (dim[0] * dim[1])
    if len(bl) != dim[0] * dim[1]:
        raise ValueError(f"{path}: BlackLevel (50714) has {len(bl)} values for BlackLevelRepeatDim {dim}")
    if len(bl) == 1:
        black = (float(bl[0]),) * 3
    else:  # by CFA position; green is the green cell on the red row (LibRaw's colour 1)
        r = cfa.index(0)
        black = (float(bl[r]), float(bl[r ^ 1]), float(bl[cfa.index(2)]))
    lin = (None,) * 4
    if linearization:
        lin = _linearization(t, raw, W, H)
    else:
        for tag in (_ID["BlackLevelDeltaH"], _ID["BlackLevelDeltaV"]):
            if any(v != 0 for v in (t.values(raw, tag, 65535) or [])):
                raise ValueError(f"{path}: {_name(tag)} with a non-zero entry is not applied")
        if _ID["LinearizationTable"] in raw:
            raise ValueError(f"{path}: LinearizationTable (50712) is not applied")
    wl =t.values(raw, _ID["WhiteLevel"], 4)
    white = float(wl[0]) if wl else float((1 << bits) - 1)

    def either(tag, max_count):
        v = t.values(ifd0, tag, max_count)
        return v if v is not None else t.values(raw, tag, max_count)

    neutral = either(_ID["AsShotNeutral"], 4)
    if neutral is None and either(_ID["AsShotWhiteXY"], 2) is not None:
        raise ValueError(f"{path}: AsShotWhiteXY (50729) without AsShotNeutral (50728) is not converted")
    wb = None
    if neutral is not None:
        if len(neutral) < 3 or any(v <= 0 for v in neutral[:3]):
            raise ValueError(f"{path}: AsShotNeutral (50728) {neutral}: three positive values expected")
        wb = [1.0 / v for v in neutral[:3]]
    cm = either(_ID["ColorMatrix1"], 12)
    if cm is not None and len(cm) != 9:
        raise ValueError(f"{path}: ColorMatrix1 (50721) has {len(cm)} values, 9 expected")
    xyz2cam = np.array(cm, np.float32).reshape(3, 3) if cm is not None else None
    npf = either(_ID["NoiseProfile"], 8)
    if npf is not None and len(npf) not in (2, 6, 8):
        raise ValueError(f"{path}: NoiseProfile (50761) has {len(npf)} values")
    ori = either(_ID["Orientation"], 1)
    iso = None
    exif_off = t.ints(ifd0, _ID["ExifIFD"], 1)
    if exif_off:
        if exif_off[0] in visited:
            raise ValueError(f"{path}: ExifIFD (34665) points at offset {exif_off[0]}, an IFD already read (a loop)")
        iso = t.ints(t.ifd(exif_off[0], "ExifIFD")[0], _ID["ISOSpeedRatings"], 3)
    if not iso:
        iso = t.ints(ifd0, _ID["ISOSpeedRatings"], 3)
    iso = min(3200, max(100, int(iso[0]))) if iso else None
    return DngInfo(path, t.byte_order, W, H, bits, comp, layout, segs, [cfa[:2], cfa[2:]], black, white, wb,
                   int(ori[0]) if ori else None, xyz2cam, npf, iso, raw_off, t.n, *lin)


# ---- lossless JPEG -------------------------------------------------------------------------------------------------------

def parse_ljpeg(stream):
    """hhsr_ljpeg_parse of one stream's bytes -> _lib.LjpegInfo; ValueError with the library's reason."""
    buf = (ctypes.c_uint8 * max(1, len(stream))).from_buffer_copy(bytes(stream) or b"\0")
    info = _lib.LjpegInfo()
    try:
        _lib.call("hhsr_ljpeg_parse", ctypes.addressof(buf), len(stream), ctypes.addressof(info))
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return info


LjpegPlan = namedtuple("LjpegPlan", "blob segments tables workspace_bytes names compressed_bytes")
LjpegPlan.__doc__ = """What hhsr_ljpeg_decode takes for a burst, in host memory: `blob` (uint8 ndarray, a multiple of 4 bytes:
the entropy-coded bytes of every stream), `segments` (ctypes array of _lib.LjpegSegment), `tables` (ctypes array of
_lib.LjpegTable, deduplicated), `workspace_bytes`, `names` ((file, index) per segment) and the streams' total bytes."""


def plan_ljpeg(files, infos):
    """The LjpegPlan of the Compression-7 files `infos` (DngInfo, one geometry) whose bytes are `files`."""
    W, H = infos[0].width, infos[0].height
    chunks, descs, names, keys, at, total = [], [], [], {}, 0, 0
    for f, (data, info) in enumerate(zip(files, infos)):
        for i, s in enumerate(info.segments):
            stream = data[s.offset:s.offset + s.length]
            try:
                lj = parse_ljpeg(stream)
            except ValueError as e:
                raise ValueError(f"{info.path}: segment {i}: {e}") from None
            if lj.P != info.bits:
                raise ValueError(f"{info.path}: segment {i}: precision {lj.P} differs from BitsPerSample (258) {info.bits}")
            if lj.X * lj.Nf * lj.Y < s.seg_w * min(s.seg_h, H - s.y0):
                raise ValueError(f"{info.path}: segment {i}: {lj.X} x {lj.Y} x {lj.Nf} samples do not fill its "
                                 f"{s.seg_w} x {s.seg_h} rectangle")
            d = _lib.LjpegSegment(offset=at, length=lj.data_length, X=lj.X, Y=lj.Y, Nf=lj.Nf, P=lj.P, predictor=lj.predictor,
                                  frame=f, x0=s.x0, y0=s.y0, seg_w=s.seg_w, seg_h=s.seg_h)
            for c in range(lj.Nf):
                th = lj.table[c]
                key = (bytes(lj.bits[th]), bytes(lj.values[th]))
                d.table[c] = keys.setdefault(key, len(keys))
            chunks.append(stream[lj.data_offset:lj.data_offset + lj.data_length])
            at += lj.data_length
            total += s.length
            descs.append(d)
            names.append((info.path, i))
    blob = np.zeros(-(-max(at, 1) // 4) * 4, np.uint8)
    blob[:at] = np.frombuffer(b"".join(chunks), np.uint8)
    segs = (_lib.LjpegSegment * len(descs))(*descs)
    bits = b"".join(k[0] for k in keys)
    values = b"".join(k[1] for k in keys)
    tables = (_lib.LjpegTable * len(keys))()
    _lib.call("hhsr_ljpeg_tables", bits, values, len(keys), ctypes.addressof(tables))
    ws = ctypes.c_size_t()
    _lib.call("hhsr_ljpeg_workspace", ctypes.addressof(segs), len(descs), ctypes.byref(ws))
    return LjpegPlan(blob, segs, tables, ws.value, names, total)


def _struct_bytes(arr):
    return np.frombuffer(arr, np.uint8, ctypes.sizeof(arr))


HOST_THREADS = 16  # the CPUs a job gets: the streams of a burst are spread over up to this many threads


def decode_ljpeg(plan, n_frames, H, W, device=None, decoder="host", threads=None):
    """The plan's streams -> uint16 counts [n_frames, H, W] on `device`, and the segments' statuses as an int32 ndarray.
    decoder "host": hhsr_ljpeg_decode_host on `threads` threads (default: min(HOST_THREADS, the CPUs of this process)),
    each a contiguous share of the streams — they write disjoint rectangles and line buffers, and ctypes releases the
    interpreter lock during the call — then the upload of the counts; "gpu": one upload of the blob, one launch of
    hhsr_ljpeg_decode."""
    n = len(plan.segments)
    if decoder == "host":
        out = np.zeros((n_frames, H, W), np.uint16)
        work = np.zeros(max(1, plan.workspace_bytes // 2), np.uint16)
        status = np.zeros(n, np.int32)
        cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        threads = max(1, min(int(threads) if threads else min(HOST_THREADS, cpus), n))
        seg_size = ctypes.sizeof(_lib.LjpegSegment)

        def share(k):
            lo, hi = k * n // threads, (k + 1) * n // threads
            if hi > lo:
                _lib.call("hhsr_ljpeg_decode_host", plan.blob.ctypes.data, plan.blob.size,
                          ctypes.addressof(plan.segments) + lo * seg_size, hi - lo, ctypes.addressof(plan.tables),
                          len(plan.tables), work.ctypes.data, work.size * 2, out.ctypes.data, n_frames, H, W, W, H * W,
                          status.ctypes.data + 4 * lo)

        if threads == 1:
            share(0)
        else:
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(share, range(threads)))
        dev = device or torch.device("cuda", torch.cuda.current_device())
        return torch.as_tensor(out).to(dev), status
    if decoder != "gpu":
        raise ValueError(f"decoder {decoder!r}: 'gpu' or 'host'")
    dev = device or torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        blob = torch.as_tensor(plan.blob).to(dev, non_blocking=True)
        segs = torch.as_tensor(_struct_bytes(plan.segments).copy()).to(dev, non_blocking=True)
        tabs = torch.as_tensor(_struct_bytes(plan.tables).copy()).to(dev, non_blocking=True)
        work = torch.empty(max(1, plan.workspace_bytes // 2), dtype=torch.uint16, device=dev)
        out = torch.zeros((n_frames, H, W), dtype=torch.uint16, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("hhsr_ljpeg_decode", _lib.ptr(blob), blob.numel(), _lib.ptr(segs), n, _lib.ptr(tabs), len(plan.tables),
                  _lib.ptr(work), work.numel() * 2, _lib.ptr(out), n_frames, H, W, W, H * W, _lib.ptr(status),
                  _lib.stream(dev))
        return out, status.cpu().numpy()


# ---- the burst ---------------------------------------------------------------------------------------------------------------

def _uncompressed(data, info):
    """The frame of an uncompressed file: uint16 counts [H, W], or for 10/12/14 bits the packed rows uint8 [H, row_bytes]."""
    W, H, e = info.width, info.height, ("<u2" if info.byte_order == "II" else ">u2")
    if info.bits == 16:
        out = np.empty((H, W), np.uint16)
        for s in info.segments:
            a = np.frombuffer(data, e, s.seg_w * s.seg_h, s.offset).reshape(s.seg_h, s.seg_w)
            h, w = min(s.seg_h, H - s.y0), min(s.seg_w, W - s.x0)
            out[s.y0:s.y0 + h, s.x0:s.x0 + w] = a[:h, :w]  # (astype to native order happens in the assignment)
        return out
    rb = packed_row_bytes(W, f"be{info.bits}")
    out = np.empty((H, rb), np.uint8)
    for s in info.segments:
        out[s.y0:s.y0 + s.seg_h] = np.frombuffer(data, np.uint8, s.seg_h * rb, s.offset).reshape(s.seg_h, rb)
    return out


def _same_linearization(a, b):
    """The name of the first linearization field in which the records a and b differ, or None."""
    for field in ("linearization_table", "black_delta_h", "black_delta_v"):
        u, v = getattr(a, field), getattr(b, field)
        if (u is None) != (v is None) or (u is not None and not np.array_equal(u, v)):
            return field
    u, v = a.gain_maps or [], b.gain_maps or []
    if len(u) != len(v) or any(m[:-1] != n[:-1] or not np.array_equal(m.gains, n.gains) for m, n in zip(u, v)):
        return "gain_maps"
    return None


def read_dng_burst(folder, device=None, decoder="host", mode="bayer", linearization=False):
    """Folder of .dng files -> the burst mapping process() takes: ``ref`` / ``comp`` as normalised float32 device tensors
    (what utils_dng.load_dng_burst returns), ``cfa_pattern``, ``white_balance``, ``iso``, ``orientation`` and ``xyz2cam`` when
    present, ``alpha`` / ``beta`` from NoiseProfile (the mean over the three planes; the first pair with `mode` "grey") and
    left out when the tag is absent, so that ``noise_model.source: estimate`` can supply them.  Files sorted by name, the
    metadata from file 0, as upstream.  Compression 7: every stream's entropy-coded bytes in one blob, decoded by the
    host function on up to 16 threads and uploaded as counts (`decoder` "host", the default: README, "Front end", has the
    measurement that decided it) or uploaded once and decoded by one launch (`decoder` "gpu", which the same measurement
    favours from about 20 frames of 12 MP on); a stream whose status is not 0 is a ValueError naming file and segment.  ``debug``: {"infos": the DngInfo records, "plan": the LjpegPlan or None}.
    `linearization=True` (``config.dng.linearization: apply``): the files are parsed with parse_dng(linearization=True); the
    table, deltas and maps of every file must equal those of file 0 (ValueError naming the file and the field); when file 0
    has any of them, the whole burst goes through utils_dng.linearize_burst in place of normalize_burst — packed 10/12/14-bit
    strips unpacked on the host first — and when it has none, through exactly the calls made without the keyword.
    ``alpha`` / ``beta`` are passed on unchanged: NoiseProfile describes the values before the gain map."""
    if decoder not in ("gpu", "host"):
        raise ValueError(f"decoder {decoder!r}: 'gpu' or 'host'")
    paths = sorted(glob.glob(os.path.join(os.fspath(folder), "*.dng")))
    if not paths:
        raise FileNotFoundError("At least one raw .dng file must be present in the burst folder.")
    infos = [parse_dng(p, linearization=True) if linearization else parse_dng(p) for p in paths]
    i0 = infos[0]
    for info in infos[1:]:
        for field in ("width", "height", "bits", "compression", "cfa_pattern"):
            if getattr(info, field) != getattr(i0, field):
                raise ValueError(f"{info.path}: {field} {getattr(info, field)} differs from {getattr(i0, field)} of {i0.path}")
        if info.compression == 1 and info.bits != 16 and info.layout != "strips":
            raise ValueError(f"{info.path}: packed tiles are not read")
        field = _same_linearization(info, i0)
        if field:
            raise ValueError(f"{info.path}: {field} differs from that of {i0.path}: one table, one pair of deltas and one set "
                             "of maps per burst")
    if i0.white_balance is None:
        raise ValueError(f"{i0.path}: AsShotNeutral (50728) is missing: no white balance")
    if i0.iso is None:
        raise AttributeError("ISO value could not be found in both EXIF and Image type.")
    files = []
    for p in paths:
        with open(p, "rb") as f:
            files.append(f.read())
    dev = device or torch.device("cuda", torch.cuda.current_device())
    levels = (i0.black_levels, i0.white_level, i0.white_balance, i0.cfa_pattern)
    plan = None
    lin = None  # what linearize_burst takes beyond the levels, when file 0 brings any of it
    if i0.linearization_table is not None or i0.black_delta_h is not None or i0.black_delta_v is not None or i0.gain_maps:
        lin = dict(table=i0.linearization_table, delta_h=i0.black_delta_h, delta_v=i0.black_delta_v, gain_maps=i0.gain_maps)

    def normalise(counts):  # (one call for the whole burst: table, deltas and maps are uploaded once)
        return linearize_burst(counts, *levels, **lin, device=dev) if lin else normalize_burst(counts, *levels, device=dev)

    if i0.compression == 7:
        plan = plan_ljpeg(files, infos)
        counts, status = decode_ljpeg(plan, len(infos), i0.height, i0.width, dev, decoder)
        bad = np.flatnonzero(status)
        if bad.size:
            path, seg = plan.names[int(bad[0])]
            raise ValueError(f"{path}: segment {seg}: lossless JPEG status {_lib.LJPEG_STATUS[int(status[bad[0]])]} "
                             f"({bad.size} of {status.size} segments failed)")
        stack = normalise(counts)
    elif i0.bits == 16:
        stack = normalise(np.stack([_uncompressed(d, i) for d, i in zip(files, infos)]))
    else:
        rows = np.stack([_uncompressed(d, i) for d, i in zip(files, infos)])
        if lin:
            # hhsr_linearize_raw_u16 takes uint16 counts only: packed strips that need it are unpacked on the HOST
            # (utils_dng.unpack_raw, NumPy).  Reading the packed layouts inside that kernel is a follow-up.
            stack = normalise(unpack_raw(rows, i0.width, f"be{i0.bits}"))
        else:
            stack = normalize_packed(rows, i0.width, f"be{i0.bits}", *levels, device=dev)
    burst = {"ref": stack[0], "comp": stack[1:], "cfa_pattern": i0.cfa_pattern, "white_balance": i0.white_balance,
             "iso": i0.iso, "debug": {"infos": infos, "plan": plan}}
    if i0.orientation is not None:
        burst["orientation"] = i0.orientation
    if i0.xyz2cam is not None:
        burst["xyz2cam"] = i0.xyz2cam
    if i0.noise_profile is not None:
        nm = i0.noise_profile
        if mode == "grey" or len(nm) == 2:
            burst.update(alpha=nm[0], beta=nm[1])
        else:
            burst.update(alpha=sum(nm[0:6:2]) / 3, beta=sum(nm[1:6:2]) / 3)
    return burst


# ---- DNG output: the container --------------------------------------------------------------------------------------------

XYZ_TO_SRGB_D65 = ((3.2404542, -1.5371385, -0.4985314), (-0.9692660, 1.8760108, 0.0415560), (0.0556434, -0.2040259, 1.0572252))
DEFAULT_CAMERA_MODEL = "handheld super-resolution"  # UniqueCameraModel of a burst that names no camera
_RATIONAL_DEN = 1000000


def _rational(x, signed):
    """(numerator, denominator) of x rounded to 10^-6; what does not fit 32 bits is a ValueError."""
    n = int(round(float(x) * _RATIONAL_DEN))
    if not (-(1 << 31) <= n < (1 << 31) if signed else 0 <= n < (1 << 32)):
        raise ValueError(f"dng_head: {x!r} does not fit a {'signed ' if signed else ''}rational with denominator {_RATIONAL_DEN}")
    return n, _RATIONAL_DEN


def dng_head(height, width, samples, tile_h, tile_w, tile_offsets=None, tile_byte_counts=None, *, orientation=1,
             camera_model=None, xyz2cam=None, white_balance=None, calibration_illuminant=None):
    """The bytes in front of the tile streams of a LinearRaw DNG (utils_dng.encode_dng): the classic little-endian TIFF
    header, IFD0 and the values it points at.  The file is ``head || streams`` with TileOffsets[i] = len(head) +
    `tile_offsets[i]`; the head's length depends only on the number of tiles and on `samples` and `camera_model`, so it is known
    before anything is coded (`tile_offsets` / `tile_byte_counts` None: zeros).  It is even, every value offset is even, the
    entries are in ascending tag order.

    IFD0: NewSubFileType 0, ImageWidth / ImageLength, BitsPerSample 16 per sample, Compression 7, PhotometricInterpretation
    34892 (LinearRaw), Orientation, SamplesPerPixel `samples` (1 or 3), PlanarConfiguration 1, TileWidth / TileLength /
    TileOffsets / TileByteCounts, DNGVersion 1.4.0.0, DNGBackwardVersion 1.1.0.0, UniqueCameraModel, BlackLevel 0 and
    WhiteLevel 65535 per sample, BaselineExposure 0; with three samples also ColorMatrix1 (`xyz2cam`; None: XYZ -> linear
    sRGB, D65), AnalogBalance (`white_balance` normalised to green; None: 1 1 1), AsShotNeutral 1 1 1 and
    CalibrationIlluminant1 (None: 21, D65).  The frames were multiplied by the white balance before the merge, so the data's
    camera space is diag(wb) ColorMatrix: AnalogBalance says exactly that (upstream's choice).  No preview IFD, no XMP, no
    NoiseProfile."""
    H, W, spp, th, tw = int(height), int(width), int(samples), int(tile_h), int(tile_w)
    if spp not in (1, 3):
        raise ValueError(f"dng_head: samples={samples!r}: 1 or 3")
    if H < 1 or W < 1 or th < 1 or tw < 1:
        raise ValueError(f"dng_head: {H} x {W} in tiles of {th} x {tw}")
    if not 1 <= int(orientation) <= 8:
        raise ValueError(f"dng_head: orientation={orientation!r}: 1 .. 8")
    n = (-(-H // th)) * (-(-W // tw))
    offs = [0] * n if tile_offsets is None else [int(v) for v in tile_offsets]
    cnts = [0] * n if tile_byte_counts is None else [int(v) for v in tile_byte_counts]
    if len(offs) != n or len(cnts) != n:
        raise ValueError(f"dng_head: {len(offs)} offsets and {len(cnts)} byte counts for {n} tiles")
    model = (DEFAULT_CAMERA_MODEL if camera_model is None else str(camera_model)).encode("ascii", "replace") + b"\0"
    BYTE, ASCII, SHORT, LONG, RATIONAL, SRATIONAL = 1, 2, 3, 4, 5, 10
    entries = [(254, LONG, [0]), (256, LONG, [W]), (257, LONG, [H]), (258, SHORT, [16] * spp), (259, SHORT, [7]),
               (262, SHORT, [34892]), (274, SHORT, [int(orientation)]), (277, SHORT, [spp]), (284, SHORT, [1]),
               (322, LONG, [tw]), (323, LONG, [th]), (324, LONG, None), (325, LONG, cnts),
               (50706, BYTE, [1, 4, 0, 0]), (50707, BYTE, [1, 1, 0, 0]), (50708, ASCII, model),
               (50714, SHORT, [0] * spp), (50717, LONG, [65535] * spp)]
    if spp == 3:
        cm = np.asarray(XYZ_TO_SRGB_D65 if xyz2cam is None else xyz2cam, np.float64).reshape(-1)
        if cm.size != 9 or not np.isfinite(cm).all():
            raise ValueError("dng_head: xyz2cam is no finite 3 x 3 matrix")
        wb = [1.0, 1.0, 1.0] if white_balance is None else [float(v) for v in np.asarray(white_balance).reshape(-1)[:3]]
        if len(wb) != 3 or not all(np.isfinite(v) and v > 0 for v in wb):
            raise ValueError(f"dng_head: white_balance={white_balance!r}: three positive values")
        illuminant = 21 if calibration_illuminant is None else int(calibration_illuminant)
        entries += [(50721, SRATIONAL, [_rational(v, True) for v in cm]),
                    (50727, RATIONAL, [_rational(v / wb[1], False) for v in wb]),
                    (50728, RATIONAL, [(1, 1)] * 3)]
    entries.append((50730, SRATIONAL, [(0, 1)]))
    if spp == 3:
        entries.append((50778, SHORT, [illuminant]))

    def payload(typ, vals):
        if typ == ASCII:
            return bytes(vals)
        if typ in (RATIONAL, SRATIONAL):
            return b"".join(struct.pack("<II" if typ == RATIONAL else "<ii", a, b) for a, b in vals)
        return struct.pack("<" + str(len(vals)) + {BYTE: "B", SHORT: "H", LONG: "I"}[typ], *vals)

    ifd_at = 8
    values_at = ifd_at + 2 + 12 * len(entries) + 4  # even: 8 + 2 + 12 k + 4
    # two passes: the first lays the values out (TileOffsets needs the head's length), the second writes them
    head_len = None
    for _ in range(2):
        body, table = b"", b""
        for tag, typ, vals in entries:
            if tag == 324:
                vals = [(head_len or 0) + o for o in offs]
                if head_len is not None and vals and max(vals) + max(cnts) >= 1 << 32:
                    raise ValueError("dng_head: the file passes 4 GiB (BigTIFF is not written)")
            data = payload(typ, vals)
            if len(data) <= 4:
                field = data + b"\0" * (4 - len(data))
            else:
                field = struct.pack("<I", values_at + len(body))
                body += data + (b"\0" if len(data) & 1 else b"")  # every value starts at an even offset
            table += struct.pack("<HHI", tag, typ, len(vals)) + field
        head_len = values_at + len(body)
    return b"II*\0" + struct.pack("<I", ifd_at) + struct.pack("<H", len(entries)) + table + struct.pack("<I", 0) + body
