"""Shared by the DNG output tests: a file (or a head) read back with Pillow's IFD reader, and its tiles decoded by
hhsr_ljpeg_parse + hhsr_ljpeg_decode_host."""
import io

import numpy as np

import ljpeg_enc_cases as enc

NAMES = {254: "NewSubFileType", 256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression",
         262: "PhotometricInterpretation", 274: "Orientation", 277: "SamplesPerPixel", 284: "PlanarConfiguration",
         322: "TileWidth", 323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 50706: "DNGVersion",
         50707: "DNGBackwardVersion", 50708: "UniqueCameraModel", 50714: "BlackLevel", 50717: "WhiteLevel",
         50721: "ColorMatrix1", 50727: "AnalogBalance", 50728: "AsShotNeutral", 50730: "BaselineExposure",
         50778: "CalibrationIlluminant1"}


def read_ifd(data):
    """{tag name: value (tuples for more than one)} of IFD0, through PIL.TiffImagePlugin.ImageFileDirectory_v2: it reads the
    IFD of a file whose photometric interpretation Pillow cannot open as an image."""
    from PIL import TiffImagePlugin

    data = bytes(data)
    ifd = TiffImagePlugin.ImageFileDirectory_v2(data[:8])
    f = io.BytesIO(data)
    f.seek(int.from_bytes(data[4:8], "little"))
    ifd.load(f)
    assert set(ifd) <= set(NAMES), sorted(set(ifd) - set(NAMES))
    return {NAMES[t]: v for t, v in dict(ifd).items()}


def raw_entries(data):
    """[(tag, type, count, value offset or None when the value is inline)] of IFD0 in file order, read with struct."""
    import struct

    data = bytes(data)
    assert data[:4] == b"II*\0"
    at = struct.unpack_from("<I", data, 4)[0]
    n = struct.unpack_from("<H", data, at)[0]
    size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 10: 8}
    out = []
    for i in range(n):
        tag, typ, count, value = struct.unpack_from("<HHII", data, at + 2 + 12 * i)
        out.append((tag, typ, count, value if size[typ] * count > 4 else None, size[typ] * count))
    assert struct.unpack_from("<I", data, at + 2 + 12 * n)[0] == 0  # no further IFD
    return out


def as_tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,)


def decode_file(data):
    """(tags, samples uint16 [H, W, Nf]) of a file of encode_dng; checks where the tiles lie."""
    data = np.asarray(data, np.uint8)
    tags = read_ifd(data)
    H, W, nf = tags["ImageLength"], tags["ImageWidth"], tags["SamplesPerPixel"]
    th, tw = tags["TileLength"], tags["TileWidth"]
    offs, cnts = as_tuple(tags["TileOffsets"]), as_tuple(tags["TileByteCounts"])
    assert len(offs) == len(cnts) == (-(-H // th)) * (-(-W // tw))
    for o, c in zip(offs, cnts):
        assert o % 2 == 0 and o + c <= data.size
        assert data[o:o + 2].tobytes() == b"\xff\xd8" and data[o + c - 2:o + c].tobytes() == b"\xff\xd9"
    return tags, enc.decode_tiles(data, offs, cnts, H, W, nf, th, tw)
