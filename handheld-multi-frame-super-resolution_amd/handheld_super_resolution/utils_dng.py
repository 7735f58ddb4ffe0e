"""Burst front end (reference utils_dng.py:50-164): sensor counts -> normalised, white-balanced
float32 RAW on the GPU.  DNG *decoding* in load_dng_burst needs rawpy + exifread like the reference; dng.py reads a folder
of .dng files without them (``config.dng.reader: native``: the container with the standard library, lossless-JPEG tiles on
the GPU) and ends in the functions below.  Bursts that are already in
memory (or in an .npz file) as integer arrays + metadata take the same normalisation without either — as uint16 counts, or
as the 10/12/14-bit packed bytes the sensor interface (MIPI CSI-2) or an uncompressed DNG holds, unpacked on the GPU."""
import ctypes

import numpy as np
import torch

from . import _lib


def to_uint16(counts):
    """Integer sensor counts, ndarray or tensor, as uint16 of the same kind; ValueError outside its range."""
    tensor = torch.is_tensor(counts)
    if (counts.numel() if tensor else counts.size) and (int(counts.min()) < 0 or int(counts.max()) > 65535):
        raise ValueError("sensor counts outside the uint16 range")
    return counts.to(torch.int32).to(torch.uint16) if tensor else counts.astype(np.uint16)


def normalize_burst(raw, black_levels, white_level, white_balance, cfa_pattern, device=None):
    """uint16 counts [n, H, W] (or [H, W]) -> float32 GPU tensor of the same shape:
    (count - black[c]) / (white - black[c]) * wb[c] / wb[1] per CFA colour c, in the reference's float32
    arithmetic (utils_dng.py:149-160).  black_levels / white_balance: per colour (R, G, B; a 4th rawpy entry for
    the second green is ignored)."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    arr = raw if isinstance(raw, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(raw))
    if arr.dtype not in (torch.uint16, torch.int16):
        if arr.dtype.is_floating_point:
            raise TypeError("normalize_burst expects integer sensor counts (got %s): float data is taken as already "
                            "normalised" % arr.dtype)
        arr = to_uint16(arr)
    squeeze = arr.dim() == 2
    if squeeze:
        arr = arr[None]
    if arr.dim() != 3:
        raise ValueError("raw must be [H, W] or [n, H, W]")
    arr = arr.contiguous().to(dev, non_blocking=True)  # current stream; does not block the host for pinned memory
    n, H, W = arr.shape
    out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    bl = [float(v) for v in list(black_levels)[:3]]
    wb = [float(v) for v in list(white_balance)[:3]]
    if len(bl) < 3 or len(wb) < 3:
        raise ValueError("black_levels and white_balance need one entry per colour (R, G, B)")
    _lib.call("hhsr_normalize_raw_u16", _lib.ptr(arr), n, H, W, W, _lib.cfa_bytes(cfa_pattern), _lib.doubles(bl),
              float(white_level), _lib.doubles(wb), _lib.ptr(out), _lib.stream())
    return out[0] if squeeze else out


def _map_field(m, name):
    return m[name] if isinstance(m, dict) else getattr(m, name)


def _map_axis(n, origin, spacing, points):
    """(i0, i1 as intp, fraction as float32) of the pixel centres of an axis of n pixels in a map of `points` points:
    include/hhsr.h, "DNG linearization", step 3."""
    i0, f = np.zeros(n, np.intp), np.zeros(n, np.float32)
    i1 = i0.copy()
    if points > 1:
        u = ((np.arange(n, dtype=np.float64) + 0.5) / np.float64(n) - np.float64(origin)) / np.float64(spacing)
        hi, mid = u >= points - 1, (u > 0) & (u < points - 1)
        fl = np.floor(u[mid])
        i0[hi] = i1[hi] = points - 1
        i0[mid], i1[mid], f[mid] = fl.astype(np.intp), fl.astype(np.intp) + 1, (u[mid] - fl).astype(np.float32)
    return i0, i1, f


def gain_map_plane(gain_map, H, W):
    """The gain of every pixel of an H x W image under one map (a dng.GainMap, or a mapping with its fields), float32
    [H, W] on the host in NumPy: the map interpolated at the pixel centres as hhsr_linearize_raw_u16 does it, operation
    by operation.  The map's Top / Left / pitches are not looked at: pixels it does not cover get the value they would have."""
    m = np.asarray(_map_field(gain_map, "gains"), np.float32)
    if m.ndim != 2:
        raise ValueError("gain_map_plane: gains must be [MapPointsV, MapPointsH]")
    r0, r1, fv = _map_axis(int(H), _map_field(gain_map, "origin_v"), _map_field(gain_map, "spacing_v"), m.shape[0])
    c0, c1, fh = _map_axis(int(W), _map_field(gain_map, "origin_h"), _map_field(gain_map, "spacing_h"), m.shape[1])
    one = np.float32(1)
    tv = m[r0] * (one - fv)[:, None] + m[r1] * fv[:, None]  # [H, PH]: the vertical blend of every map column
    return tv[:, c0] * (one - fh)[None, :] + tv[:, c1] * fh[None, :]


def linearize_burst(raw, black_levels, white_level, white_balance, cfa_pattern, table=None, delta_h=None, delta_v=None,
                    gain_maps=None, device=None):
    """normalize_burst() with a DNG's LinearizationTable (`table`: up to 65536 uint16 entries), BlackLevelDeltaH / V
    (`delta_h` [W], `delta_v` [H], float32) and GainMap opcodes (`gain_maps`: up to four dng.GainMap records or mappings
    with their fields — one with pitches 1, or one per 2 x 2 position with pitches 2) applied on the GPU
    (hhsr_linearize_raw_u16; include/hhsr.h states every operation).  The same input forms as normalize_burst; table,
    deltas and gains may be device tensors already (read_dng_burst uploads them once).  With all four absent the result
    equals normalize_burst's for integer levels.  NoiseProfile describes the values BEFORE the gain map: a map scales the
    noise with the position, which nothing downstream models."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    arr = raw if isinstance(raw, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(raw))
    if arr.dtype not in (torch.uint16, torch.int16):
        if arr.dtype.is_floating_point:
            raise TypeError("linearize_burst expects integer sensor counts (got %s): float data is taken as already "
                            "normalised" % arr.dtype)
        arr = to_uint16(arr)
    squeeze = arr.dim() == 2
    if squeeze:
        arr = arr[None]
    if arr.dim() != 3:
        raise ValueError("raw must be [H, W] or [n, H, W]")
    arr = arr.contiguous().to(dev, non_blocking=True)
    n, H, W = arr.shape
    bl = [float(v) for v in list(black_levels)[:3]]
    wb = [float(v) for v in list(white_balance)[:3]]
    if len(bl) < 3 or len(wb) < 3:
        raise ValueError("black_levels and white_balance need one entry per colour (R, G, B)")

    def vector(v, dtype, np_dtype, length, name):
        if v is None:
            return None
        if not torch.is_tensor(v):
            a = np.asarray(v)
            if np_dtype == np.uint16 and (not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 65535))):
                raise ValueError(f"linearize_burst: {name} must hold integers in 0 .. 65535")
            v = torch.as_tensor(np.ascontiguousarray(a.astype(np_dtype)))
        if v.dim() != 1 or v.dtype not in ((torch.uint16, torch.int16) if np_dtype == np.uint16 else (dtype,)):
            raise ValueError(f"linearize_burst: {name} must be a 1-D {np.dtype(np_dtype).name} array")
        if not (v.numel() == length if length else 1 <= v.numel() <= 65536):
            raise ValueError(f"linearize_burst: {name} has {v.numel()} entries" + (f", {length} expected" if length else ""))
        return v.contiguous().to(dev, non_blocking=True)

    tab = vector(table, torch.uint16, np.uint16, None, "table")
    dh = vector(delta_h, torch.float32, np.float32, W, "delta_h")
    dv = vector(delta_v, torch.float32, np.float32, H, "delta_v")
    maps = list(gain_maps or [])
    if len(maps) > _lib.MAX_GAIN_MAPS:
        raise ValueError(f"linearize_burst: {len(maps)} gain maps, at most {_lib.MAX_GAIN_MAPS}")
    descs, at, pieces = (_lib.GainMapDesc * max(1, len(maps)))(), 0, []
    for i, m in enumerate(maps):
        g = _map_field(m, "gains")
        g = g if torch.is_tensor(g) else torch.as_tensor(np.ascontiguousarray(g, np.float32))
        if g.dim() != 2 or g.dtype != torch.float32:
            raise ValueError("linearize_burst: a map's gains must be float32 [MapPointsV, MapPointsH]")
        descs[i] = _lib.GainMapDesc(*(int(_map_field(m, k)) for k in ("top", "left", "row_pitch", "col_pitch")), g.shape[0],
                                    g.shape[1], *(float(_map_field(m, k)) for k in ("spacing_v", "spacing_h", "origin_v",
                                                                                   "origin_h")), at)
        at += g.numel()
        pieces.append(g.reshape(-1).to(dev, non_blocking=True))
    gains = torch.cat(pieces) if pieces else None
    out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    _lib.call("hhsr_linearize_raw_u16", _lib.ptr(arr), n, H, W, W, _lib.cfa_bytes(cfa_pattern), _lib.doubles(bl),
              float(white_level), _lib.doubles(wb), _lib.ptr(tab), tab.numel() if tab is not None else 0, _lib.ptr(dh),
              _lib.ptr(dv), ctypes.addressof(descs) if maps else None, len(maps), _lib.ptr(gains), at, _lib.ptr(out),
              _lib.stream())
    return out[0] if squeeze else out


# Packed layouts of hhsr_normalize_raw_packed (include/hhsr.h states them operation by operation): name -> id
PACKINGS = {"mipi10": 1, "mipi12": 2, "mipi14": 3, "be10": 4, "be12": 5, "be14": 6}


def _packing(packing):
    """(id, bits, big-endian bit stream?) of a layout given by name or id."""
    pid = PACKINGS.get(packing) if isinstance(packing, str) else (int(packing) if int(packing) in PACKINGS.values() else None)
    if pid is None:
        raise ValueError(f"packing {packing!r}: one of {sorted(PACKINGS)}")
    return pid, 10 + 2 * ((pid - 1) % 3), pid >= 4


def packed_row_bytes(width, packing):
    """Bytes one packed row of `width` pixels occupies (the library's rule: hhsr_packed_row_bytes, no GPU needed)."""
    out = ctypes.c_int64()
    _lib.call("hhsr_packed_row_bytes", int(width), _packing(packing)[0], ctypes.byref(out))
    return out.value


def pack_raw(counts, packing, row_bytes=None):
    """Integer counts [..., W] -> uint8 [..., row_bytes] in a packed layout (NumPy, on the host: fixtures, tests, tools).
    Padding pixels of the last group, trailing bits and the bytes up to `row_bytes` (default: the minimum) are zero."""
    pid, bits, be = _packing(packing)
    p = np.asarray(counts)
    if not np.issubdtype(p.dtype, np.integer) or p.ndim < 1:
        raise TypeError("pack_raw expects integer counts [..., W]")
    if p.size and (int(p.min()) < 0 or int(p.max()) >= 1 << bits):
        raise ValueError(f"counts outside the {bits}-bit range")
    p = p.astype(np.uint32)
    W = p.shape[-1]
    if be:
        stream = ((p[..., None] >> np.arange(bits - 1, -1, -1, dtype=np.uint32)) & 1).astype(np.uint8)
        rows = np.packbits(stream.reshape(*p.shape[:-1], W * bits), axis=-1)
    else:
        G, lb = (2 if bits == 12 else 4), bits - 8
        g = np.zeros((*p.shape[:-1], -(-W // G) * G), np.uint32)
        g[..., :W] = p
        g = g.reshape(*p.shape[:-1], -1, G)
        low = ((g & ((1 << lb) - 1)) << (lb * np.arange(G, dtype=np.uint32))).sum(axis=-1, dtype=np.uint32)
        low = (low[..., None] >> (8 * np.arange(G * lb // 8, dtype=np.uint32))) & 255  # little-endian
        rows = np.concatenate([g >> lb, low], axis=-1).astype(np.uint8).reshape(*p.shape[:-1], -1)
    need = packed_row_bytes(W, pid)
    assert rows.shape[-1] == need, (rows.shape, need)
    if row_bytes is None or int(row_bytes) == need:
        return np.ascontiguousarray(rows)
    if int(row_bytes) < need:
        raise ValueError(f"row_bytes {row_bytes} < {need}, the bytes of {W} pixels")
    out = np.zeros((*rows.shape[:-1], int(row_bytes)), np.uint8)
    out[..., :need] = rows
    return out


def unpack_raw(packed, width, packing):
    """uint8 [..., row_bytes] -> uint16 counts [..., width]: the restated reference of the layouts (NumPy, host)."""
    pid, bits, be = _packing(packing)
    b = np.asarray(packed)
    need = packed_row_bytes(width, pid)
    if b.dtype != np.uint8 or b.ndim < 1 or b.shape[-1] < need:
        raise ValueError(f"unpack_raw expects uint8 [..., >= {need}] for {width} pixels")
    b = b[..., :need]
    if be:
        stream = np.unpackbits(b, axis=-1)[..., :width * bits].reshape(*b.shape[:-1], width, bits)
        p = (stream.astype(np.uint32) << np.arange(bits - 1, -1, -1, dtype=np.uint32)).sum(axis=-1, dtype=np.uint32)
    else:
        G, lb = (2 if bits == 12 else 4), bits - 8
        g = b.reshape(*b.shape[:-1], -1, G + G * lb // 8).astype(np.uint32)
        low = (g[..., G:] << (8 * np.arange(G * lb // 8, dtype=np.uint32))).sum(axis=-1, dtype=np.uint32)
        p = (g[..., :G] << lb) | ((low[..., None] >> (lb * np.arange(G, dtype=np.uint32))) & ((1 << lb) - 1))
        p = p.reshape(*b.shape[:-1], -1)[..., :width]
    return p.astype(np.uint16)


def infer_width(row_bytes, packing):
    """The width whose packed rows are exactly `row_bytes` long with no padding pixel or bit, or None."""
    _, bits, be = _packing(packing)
    per, px = (bits, 8) if be else ((3, 2) if bits == 12 else (bits // 2, 4))  # `per` bytes hold `px` pixels
    return row_bytes * px // per if row_bytes > 0 and (row_bytes * px) % per == 0 else None


def normalize_packed(raw_u8, width, packing, black_levels, white_level, white_balance, cfa_pattern, device=None):
    """Packed counts uint8 [n, H, row_bytes] (or [H, row_bytes]) -> float32 GPU tensor [n, H, width] (or [H, width]):
    normalize_burst() of the unpacked counts, bit for bit, without unpacking them on the host (hhsr_normalize_raw_packed).
    Host data is uploaded as it is on the current stream; rows may be longer than packed_row_bytes(width, packing)."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    pid = _packing(packing)[0]
    arr = raw_u8 if isinstance(raw_u8, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(raw_u8))
    if arr.dtype != torch.uint8:
        raise TypeError("normalize_packed expects the packed bytes as uint8 (got %s)" % arr.dtype)
    squeeze = arr.dim() == 2
    if squeeze:
        arr = arr[None]
    if arr.dim() != 3:
        raise ValueError("raw must be [H, row_bytes] or [n, H, row_bytes]")
    arr = arr.contiguous().to(dev, non_blocking=True)  # current stream; does not block the host for pinned memory
    n, H, row_bytes = arr.shape
    out = torch.empty((n, H, int(width)), dtype=torch.float32, device=dev)
    bl = [float(v) for v in list(black_levels)[:3]]
    wb = [float(v) for v in list(white_balance)[:3]]
    if len(bl) < 3 or len(wb) < 3:
        raise ValueError("black_levels and white_balance need one entry per colour (R, G, B)")
    _lib.call("hhsr_normalize_raw_packed", _lib.ptr(arr), n, H, int(width), row_bytes, H * row_bytes, pid,
              _lib.cfa_bytes(cfa_pattern), _lib.doubles(bl), float(white_level), _lib.doubles(wb), _lib.ptr(out),
              _lib.stream())
    return out[0] if squeeze else out


def load_dng_burst(burst_path):
    """Folder of .dng files -> (ref_raw, raw_comp, ISO, tags, CFA, xyz2cam, white_balance, ref_path) like the
    reference (utils_dng.py:50-164), with the normalisation done on the GPU.  Needs rawpy + exifread."""
    try:
        import rawpy
        import exifread
    except ImportError as e:
        raise ImportError("reading .dng bursts needs rawpy and exifread (not installed); pass an in-memory burst "
                          "or an .npz file instead") from e
    import glob
    import os

    paths = sorted(glob.glob(os.path.join(str(burst_path), "*.dng")))
    if not paths:
        raise FileNotFoundError("At least one raw .dng file must be present in the burst folder.")
    frames = []
    for p in paths:
        with rawpy.imread(p) as ro:
            frames.append(ro.raw_image.copy())
    with rawpy.imread(paths[0]) as raw:
        white_level = int(raw.white_level)
        black_levels = list(raw.black_level_per_channel)
        white_balance = list(raw.camera_whitebalance)
        cfa = raw.raw_pattern.copy()
    cfa[cfa == 3] = 1
    with open(paths[0], "rb") as f:
        tags = exifread.process_file(f)
    if "EXIF ISOSpeedRatings" in tags:
        iso = int(str(tags["EXIF ISOSpeedRatings"]))
    elif "Image ISOSpeedRatings" in tags:
        iso = int(str(tags["Image ISOSpeedRatings"]))
    else:
        raise AttributeError("ISO value could not be found in both EXIF and Image type.")
    iso = min(3200, max(100, iso))
    xyz2cam = None
    if "Image Tag 0xC621" in tags:  # DNG ColorMatrix1 (raw2rgb.py:11-26)
        xyz2cam = np.array([x.decimal() for x in tags["Image Tag 0xC621"].values]).reshape(3, 3).astype(np.float32)
    stack = normalize_burst(np.stack(frames), black_levels, white_level, white_balance, cfa)
    return stack[0], stack[1:], iso, tags, cfa, xyz2cam, white_balance, paths[0]


TIFF_MAX_BYTES = 2 ** 32 - 1  # classic TIFF: 32-bit offsets


def save_as_tiff(int_im, outpath):
    """uint8 / uint16 ndarray [H, W] or [H, W, 3] -> baseline TIFF (reference utils_dng.py:327-341, which writes it through
    imageio with bigtiff=False): little-endian, uncompressed, one strip, chunky, standard library only.  A path that does
    not end in .tif / .tiff gets the suffix .tif, as upstream.  RuntimeError when the file would pass classic TIFF's 4 GiB,
    like the reference."""
    import os
    import struct

    a = np.asarray(int_im)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"save_as_tiff expects uint8 / uint16 [H, W] or [H, W, 3], got {a.dtype} {a.shape}")
    path = os.fspath(outpath)
    if os.path.splitext(path)[1].lower() not in (".tif", ".tiff"):
        path = os.path.splitext(path)[0] + ".tif"
    H, W = a.shape[:2]
    spp, bits = (3 if a.ndim == 3 else 1), 8 * a.dtype.itemsize
    nbytes = _tiff_pixel_bytes(a)
    SHORT, LONG, RATIONAL = 3, 4, 5
    # header (8) | BitsPerSample x 3 (6, RGB only) + pad (2) | XResolution, YResolution (16) | IFD | pixels
    bps_off, res_off, ifd_off = 8, 16, 32
    tags = [(256, LONG, 1, W), (257, LONG, 1, H), (258, SHORT, spp, bps_off if spp == 3 else bits), (259, SHORT, 1, 1),
            (262, SHORT, 1, 2 if spp == 3 else 1), (273, LONG, 1, 0), (277, SHORT, 1, spp), (278, LONG, 1, H),
            (279, LONG, 1, nbytes), (282, RATIONAL, 1, res_off), (283, RATIONAL, 1, res_off + 8), (284, SHORT, 1, 1),
            (296, SHORT, 1, 2)]
    data_off = ifd_off + 2 + 12 * len(tags) + 4
    if data_off + nbytes > TIFF_MAX_BYTES:
        raise RuntimeError(f"{os.path.basename(path)!r}: {data_off + nbytes} bytes are too large for a classic TIFF, whose "
                           f"offsets are 32-bit (4 GiB); BigTIFF is not written.")
    head = struct.pack("<2sHI", b"II", 42, ifd_off) + struct.pack("<4H", bits, bits, bits, 0)
    head += struct.pack("<4I", 72, 1, 72, 1) + struct.pack("<H", len(tags))
    for tag, typ, count, value in tags:
        if tag == 273:
            value = data_off
        if typ == SHORT and count == 1:
            head += struct.pack("<HHIHH", tag, typ, count, value, 0)
        else:
            head += struct.pack("<HHII", tag, typ, count, value)
    head += struct.pack("<I", 0)  # no further IFD
    assert len(head) == data_off
    with open(path, "wb") as f:
        f.write(head)
        f.write(np.ascontiguousarray(a.astype("<u2") if a.dtype == np.uint16 else a).tobytes())


def _tiff_pixel_bytes(a):
    """Bytes of the one strip (its own function: the 4 GiB refusal is tested without allocating 4 GiB)."""
    return int(a.size) * a.dtype.itemsize


# ---- DNG output (include/hhsr.h "DNG output: lossless JPEG"; the reference's save_as_dng runs exiftool and dng_validate) -------
DNG_TILE = 128      # default tile edge, chosen by measurement (profiles/dng_encode.txt, 48 MP): the fastest of 128 / 256 / 512
#                     whose file is within 1 % of the smallest of the three.  128 is both: 2961 workgroups fill the chip where
#                     768 or 192 do not, and the replicated rows below the image, which predictor 1 codes at full cost, are fewest
DNG_PREDICTOR = 1   # what DNG writers use; the decoder keeps it out of its switch


def dng_option(name, value):
    """The canonical value of an encode_dng / config.output option: tile -> (tile_h, tile_w), each a multiple of 16 in
    16 .. 65535, from one integer or a pair (None: DNG_TILE square); predictor -> an int in 1 .. 7 (None: DNG_PREDICTOR).
    Anything else is a ValueError."""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))

    if name == "tile":
        if value is None:
            return DNG_TILE, DNG_TILE
        pair = [value, value] if integer(value) else list(value) if hasattr(value, "__len__") and not isinstance(value, str) else None
        if pair is None or len(pair) != 2 or not all(integer(v) and 16 <= int(v) <= 65535 and int(v) % 16 == 0 for v in pair):
            raise ValueError(f"tile={value!r}: one integer or [h, w], each a multiple of 16 in 16 .. 65535")
        return int(pair[0]), int(pair[1])
    if name == "predictor":
        if value is None:
            return DNG_PREDICTOR
        if not integer(value) or not 1 <= int(value) <= 7:
            raise ValueError(f"predictor={value!r}: an integer in 1 .. 7")
        return int(value)
    raise ValueError(f"dng_option: no option {name!r}")


def ljpeg_encode_workspace(H, W, Nf, tile_h, tile_w):
    """(bytes of the scratch, largest possible result) of hhsr_ljpeg_encode_workspace."""
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.call("hhsr_ljpeg_encode_workspace", int(H), int(W), int(Nf), int(tile_h), int(tile_w), ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def ljpeg_huffman(counts):
    """hhsr_ljpeg_huffman per row of counts [Nf, 17] (host) -> (bits uint8 [Nf, 16], values uint8 [Nf, 17]): T.81 Annex K.2."""
    c = np.ascontiguousarray(counts, np.uint64)
    if c.ndim != 2 or c.shape[1] != 17 or not 1 <= c.shape[0] <= 4:
        raise ValueError(f"ljpeg_huffman expects counts [Nf, 17], got {c.shape}")
    bits, values, n = np.zeros((c.shape[0], 16), np.uint8), np.zeros((c.shape[0], 17), np.uint8), ctypes.c_int(0)
    for i in range(c.shape[0]):
        _lib.call("hhsr_ljpeg_huffman", c[i].ctypes.data, bits[i].ctypes.data, values[i].ctypes.data, ctypes.byref(n))
    return bits, values


def encode_dng(img, *, channels=None, tile=None, predictor=None, xyz2cam=None, white_balance=None, orientation=1,
               camera_model=None, calibration_illuminant=None, capacity=None):
    """Device float32 [H, W, 3] or [H, W] -> the complete LinearRaw DNG file as a 1-D uint8 ndarray: the samples of
    encode_image(img, "uint16") in tiles of `tile` (one integer or (h, w); default DNG_TILE), each one lossless-JPEG stream
    (Compression 7, `predictor` 1 .. 7) coded on the device with Huffman tables made for this image, behind the container of
    dng.dng_head (which documents the tags and what `xyz2cam`, `white_balance`, `orientation`, `camera_model` and
    `calibration_illuminant` become).  `channels=1` of an [H, W, 3] image: channel 0 alone, one sample per pixel (`mode: grey`).
    Two synchronisations, as encode_png: the Nf x 17 category counts are copied (hhsr_ljpeg_histogram), hhsr_ljpeg_huffman
    builds one table per component on the host, the streams are coded into `capacity` device bytes (default: the size of
    the uncompressed samples plus 256 bytes per tile), the offsets, byte counts and the length are read, and exactly the
    streams' bytes are copied behind the head; a result that did not fit is coded once more into a buffer of the reported
    length."""
    from .dng import dng_head
    from .utils_image import encode_image

    if not (torch.is_tensor(img) and img.is_cuda):
        raise RuntimeError("encode_dng expects a tensor on the GPU (the HIP path has no CPU fallback)")
    tile_h, tile_w = dng_option("tile", tile)
    predictor = dng_option("predictor", predictor)
    samples = encode_image(img, "uint16", channels=channels)  # (checks the shape; int16 storage of the uint16 samples)
    H, W = samples.shape[:2]
    nf = 1 if samples.dim() == 2 else samples.shape[2]
    dev, stream = samples.device, _lib.stream(samples.device)
    n_tiles = (-(-H // tile_h)) * (-(-W // tile_w))
    meta = dict(orientation=orientation, camera_model=camera_model, xyz2cam=xyz2cam, white_balance=white_balance,
                calibration_illuminant=calibration_illuminant)
    head_len = len(dng_head(H, W, nf, tile_h, tile_w, **meta))  # (also refuses what the container cannot hold, before any launch)
    scratch_bytes, _ = ljpeg_encode_workspace(H, W, nf, tile_h, tile_w)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(nf * 17 + 1, dtype=torch.int64, device=dev)  # [Nf][17], then the status word
    args = (_lib.ptr(samples), H, W, nf, W * nf, 16, predictor, tile_h, tile_w)
    _lib.call("hhsr_ljpeg_histogram", *args, _lib.ptr(counts), ctypes.c_void_p(counts.data_ptr() + 8 * nf * 17),
              _lib.ptr(scratch), scratch.numel() * 8, stream)
    bits, values = ljpeg_huffman(counts.cpu().numpy().view(np.uint64)[:nf * 17].reshape(nf, 17))  # (synchronises: the counts)
    record = torch.empty(n_tiles + 2 + (n_tiles + 1) // 2, dtype=torch.int64, device=dev)  # offsets, length, byte counts
    p_off = record.data_ptr()
    p_len, p_cnt = p_off + 8 * (n_tiles + 1), p_off + 8 * (n_tiles + 2)
    cap = H * W * nf * 2 + 256 * n_tiles if capacity is None else int(capacity)
    for _ in range(2):  # at most one retry, with the length the first pass reported
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        _lib.call("hhsr_ljpeg_encode", *args, bits.ctypes.data, values.ctypes.data, _lib.ptr(scratch), scratch.numel() * 8,
                  _lib.ptr(out), cap, ctypes.c_void_p(p_off), ctypes.c_void_p(p_cnt), ctypes.c_void_p(p_len), stream)
        rec = record.cpu().numpy()  # (synchronises: 12 bytes per tile)
        offsets = rec[:n_tiles + 1].view(np.uint64)
        byte_counts = rec[n_tiles + 2:].view(np.uint32)[:n_tiles]
        length = int(rec[n_tiles + 1:n_tiles + 2].view(np.uint64)[0])
        if length == (1 << 64) - 1:  # (cannot happen with tables built from this image's counts)
            raise RuntimeError("encode_dng: the Huffman tables lack a category the image holds")
        if length <= cap:
            break
        cap = length
    else:
        raise RuntimeError(f"encode_dng: the streams need {length} bytes after a retry with the reported length")
    head = dng_head(H, W, nf, tile_h, tile_w, offsets[:n_tiles], byte_counts, **meta)
    assert len(head) == head_len
    data = np.empty(head_len + length, np.uint8)
    data[:head_len] = np.frombuffer(head, np.uint8)
    torch.from_numpy(data)[head_len:].copy_(out[:length])  # (device -> its place in the file: one host copy)
    return data


def save_dng_bytes(file_bytes, path):
    """The array encode_dng (or process() with output.format = dng) returned -> a file."""
    a = np.asarray(file_bytes)
    if a.dtype != np.uint8 or a.ndim != 1 or a.size < 8 or a[:4].tobytes() != b"II*\0":
        raise ValueError("save_dng_bytes expects the 1-D uint8 array of encode_dng")
    with open(path, "wb") as f:
        f.write(a.tobytes())


def save_as_dng(np_img, ref_dng_path, outpath):
    """The reference's signature (utils_dng.py:218-325): the linear image `np_img` (float [H, W, 3] or [H, W], host or
    device) as a DNG at `outpath`, with the colour matrix, white balance and orientation of `ref_dng_path` read by
    dng.parse_dng.  Upstream writes a 16-bit TIFF and rewrites its tags with exiftool, then runs dng_validate; here the file
    is coded on the GPU (encode_dng) and neither tool is needed."""
    from .dng import parse_dng

    info = parse_dng(ref_dng_path)
    img = np_img if torch.is_tensor(np_img) else torch.as_tensor(np.ascontiguousarray(np_img, np.float32))
    data = encode_dng(_lib.f32c(img), xyz2cam=info.xyz2cam, white_balance=info.white_balance,
                      orientation=info.orientation or 1)
    save_dng_bytes(data, outpath)
