"""A DNG writer for the tests, standard library + NumPy: II / MM, the raw IFD in IFD0 or in a SubIFD behind a thumbnail
IFD0, strips or tiles, Compression 1 at 16 / 10 / 12 / 14 bits or Compression 7 (tests/ljpeg_ref.py), and the tags
handheld_super_resolution.dng reads.  `extra` / `drop` change single tags of the raw IFD or IFD0 for the refusal tests."""
import struct

import numpy as np

import ljpeg_ref

BYTE, ASCII, SHORT, LONG, RATIONAL, SRATIONAL, DOUBLE = 1, 2, 3, 4, 5, 10, 12
_FMT = {BYTE: "B", SHORT: "H", LONG: "I", DOUBLE: "d"}


def _rational(v, signed=False):
    den = 1000000
    return int(round(v * den)), den


def _payload(e, typ, values):
    if typ in (RATIONAL, SRATIONAL):
        flat = [x for v in values for x in _rational(v)]
        return struct.pack(e + str(len(flat)) + ("I" if typ == RATIONAL else "i"), *flat)
    if typ == ASCII:
        return bytes(values)
    return struct.pack(e + str(len(values)) + _FMT[typ], *values)


def pack_be(counts, bits):
    """Rows of counts [h, W] as TIFF's MSB-first bit stream, every row starting on a byte."""
    p = np.asarray(counts).astype(np.uint32)
    stream = ((p[..., None] >> np.arange(bits - 1, -1, -1, dtype=np.uint32)) & 1).astype(np.uint8)
    return np.packbits(stream.reshape(p.shape[0], -1), axis=-1)


class Writer:
    """Lays out IFDs and data blocks; offsets are assigned when the file is assembled."""

    def __init__(self, byte_order="II"):
        self.e = "<" if byte_order == "II" else ">"
        self.bo = byte_order
        self.buf = bytearray(self.bo.encode() + struct.pack(self.e + "HI", 42, 0))

    def block(self, data):
        """Append a data block on an even offset; its offset."""
        if len(self.buf) % 2:
            self.buf += b"\0"
        off = len(self.buf)
        self.buf += data
        return off

    def ifd(self, entries, next_ifd=0):
        """Append an IFD of (tag, type, values) entries (values: list, or bytes for ASCII); its offset."""
        ents = []
        for tag, typ, values in sorted(entries, key=lambda t: t[0]):
            pay = _payload(self.e, typ, values)
            count = len(values) if typ != ASCII else len(pay)
            if len(pay) <= 4:
                ents.append((tag, typ, count, pay.ljust(4, b"\0"), None))
            else:
                ents.append((tag, typ, count, None, self.block(pay)))
        if len(self.buf) % 2:
            self.buf += b"\0"
        off = len(self.buf)
        self.buf += struct.pack(self.e + "H", len(ents))
        for tag, typ, count, inline, at in ents:
            self.buf += struct.pack(self.e + "HHI", tag, typ, count)
            self.buf += inline if inline is not None else struct.pack(self.e + "I", at)
        self.buf += struct.pack(self.e + "I", next_ifd)
        return off

    def finish(self, first_ifd):
        struct.pack_into(self.e + "I", self.buf, 4, first_ifd)
        return bytes(self.buf)


def raw_segments(counts, bits, compression, layout, size, byte_order, ljpeg):
    """([bytes per strip / tile], layout tags) of counts [H, W]."""
    H, W = counts.shape
    if layout == "tiles":
        tw, th = size
        rects = [(x0, y0, tw, th) for y0 in range(0, H, th) for x0 in range(0, W, tw)]
    else:
        rects = [(0, y0, W, min(size, H - y0)) for y0 in range(0, H, size)]
    out = []
    for x0, y0, w, h in rects:
        rect = counts[y0:y0 + h, x0:x0 + w]
        rect = np.pad(rect, ((0, h - rect.shape[0]), (0, w - rect.shape[1])), mode="edge")
        if compression == 7:
            nf = ljpeg.get("Nf", 1)
            x = ljpeg.get("X", w // nf)
            out.append(ljpeg_ref.encode(ljpeg_ref.to_stream_geometry(rect, nf, x), bits, ljpeg.get("predictor", 1),
                                        tables=ljpeg.get("tables", "k2")))
        elif bits == 16:
            out.append(rect.astype("<u2" if byte_order == "II" else ">u2").tobytes())
        else:
            out.append(pack_be(rect, bits).tobytes())
    return out, rects


def write_dng(path, counts, bits=16, byte_order="II", subifd=False, layout="strips", size=None, compression=1,
              cfa=(0, 1, 1, 2), black=(64, 65, 66, 67), white=None, neutral=(0.5, 1.0, 0.625), color_matrix=None,
              noise_profile=None, iso=400, iso_in_exif=True, orientation=1, ljpeg=None, extra=(), extra0=(), drop=(),
              big=False):
    """counts [H, W] -> a DNG file at `path`; returns the dict of what was written (the tests' expectation).
    black: one value, or four by CFA position.  extra / extra0: (tag, type, values) entries that replace or join those of
    the raw IFD / IFD0; drop: tags left out of either."""
    counts = np.asarray(counts)
    H, W = counts.shape
    size = size if size is not None else ((64, 32) if layout == "tiles" else 16)
    white = (1 << bits) - 1 if white is None else white
    w = Writer(byte_order)
    datas, rects = raw_segments(counts, bits, compression, layout, size, byte_order, ljpeg or {})
    offs = [w.block(d) for d in datas]
    black = list(black) if hasattr(black, "__len__") else [black]
    raw = [(254, LONG, [0]), (256, LONG, [W]), (257, LONG, [H]), (258, SHORT, [bits]), (259, SHORT, [compression]),
           (262, SHORT, [32803]), (277, SHORT, [1]), (284, SHORT, [1]), (33421, SHORT, [2, 2]), (33422, BYTE, list(cfa)),
           (50713, SHORT, [2, 2] if len(black) == 4 else [1, 1]), (50714, RATIONAL, black), (50717, LONG, [white])]
    if layout == "tiles":
        raw += [(322, LONG, [size[0]]), (323, LONG, [size[1]]), (324, LONG, offs), (325, LONG, [len(d) for d in datas])]
    else:
        raw += [(278, LONG, [size]), (273, LONG, offs), (279, LONG, [len(d) for d in datas])]
    shared = [(50706, BYTE, [1, 4, 0, 0]), (274, SHORT, [orientation])]
    if neutral is not None:
        shared.append((50728, RATIONAL, list(neutral)))
    if color_matrix is not None:
        shared.append((50721, SRATIONAL, [float(v) for v in np.asarray(color_matrix).reshape(-1)]))
    if noise_profile is not None:
        shared.append((50761, DOUBLE, [float(v) for v in noise_profile]))
    if iso is not None:
        if iso_in_exif:
            shared.append((34665, LONG, [w.ifd([(34855, SHORT, [iso])])]))
        else:
            shared.append((34855, SHORT, [iso]))

    def merged(base, more):
        keep = {t[0]: t for t in base if t[0] not in drop}
        keep.update({t[0]: t for t in more})
        return list(keep.values())

    if subifd:
        thumb = np.zeros((4, 6, 3), np.uint8).tobytes()
        sub = w.ifd(merged(raw, extra))
        ifd0 = [(254, LONG, [1]), (256, LONG, [6]), (257, LONG, [4]), (258, SHORT, [8, 8, 8]), (259, SHORT, [1]),
                (262, SHORT, [2]), (273, LONG, [w.block(thumb)]), (277, SHORT, [3]), (278, LONG, [4]), (279, LONG, [len(thumb)]),
                (330, LONG, [sub])] + shared
        first = w.ifd(merged(ifd0, extra0))
    else:
        first = w.ifd(merged(raw + shared, list(extra) + list(extra0)))
    data = w.finish(first)
    if big:
        data = data[:2] + struct.pack(w.e + "H", 43) + data[4:]
    with open(path, "wb") as f:
        f.write(data)
    r = cfa.index(0)
    bl = (black * 4)[:4] if len(black) == 1 else black
    return {"width": W, "height": H, "bits": bits, "compression": compression, "layout": layout, "byte_order": byte_order,
            "cfa_pattern": [list(cfa[:2]), list(cfa[2:])], "black_levels": (float(bl[r]), float(bl[r ^ 1]), float(bl[cfa.index(2)])),
            "white_level": float(white), "white_balance": None if neutral is None else [1.0 / v for v in neutral],
            "iso": None if iso is None else min(3200, max(100, iso)), "orientation": orientation,
            "n_segments": len(datas), "rects": rects, "offsets": offs, "lengths": [len(d) for d in datas], "bytes": data}
