"""White-balance gains (R, 1, B) of a Bayer burst that brings none, estimated from its sensor counts.  The reference takes
rawpy's camera_whitebalance (DNG AsShotNeutral, utils_dng.py:149-160); uint16 counts and packed rows from a sensor interface
have no such tag.

The statistic is one pass over the frames as they lie in HBM (hhsr_white_balance_hist): per whole 16 x 16 pixel tile the
integer sums of the three colours, the normalised means and the two chroma quotients m_G / m_R and m_G / m_B, binned at 32
bins per octave into an integer histogram [192, 192]; clipped and dark tiles are dropped.  The fit is host code of the same
library (hhsr_white_balance_fit): the count-weighted centroid of the bin centres in log2 units — a geometric grey world —
refined four times inside a gate of half an octave, which throws out a large coloured object.  include/hhsr.h states both,
tests/white_balance_ref.py is their NumPy form.

Grey world's own assumption is not corrected and cannot be: a scene whose balanced channel means differ is estimated wrong
by that difference."""
import ctypes as C

import numpy as np
import torch

from . import _lib

BINS = 192  # HHSR_WB_BINS
HIST_SHAPE = (BINS, BINS)
SOURCES = ("given", "estimate")
MIN_TILES = 16


def wb_options(config):
    """(source, frames, min_tiles) of the optional section config.white_balance = {"source": "given" | "estimate",
    "frames": 1, "min_tiles": 16} (not in the reference schema, like config.reference and config.output; absent:
    ("given", 1, 16)).  frames: how many frames of the burst, from the reference frame on, are measured.  ValueError for
    anything else."""
    sec = config.get("white_balance", None) or {}
    source = str(sec.get("source", "given"))
    if source not in SOURCES:
        raise ValueError(f"config.white_balance.source {source!r}: given or estimate")
    out = []
    for key, default in (("frames", 1), ("min_tiles", MIN_TILES)):
        v = sec.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"config.white_balance.{key} {v!r}: an integer >= 1")
        out.append(int(v))
    return source, out[0], out[1]


def white_balance_histogram(frames, cfa_pattern, black_levels, white_level, packing=None, width=None):
    """Tile histogram of a list of device frames of one shape -> device int32 tensor [192, 192] holding the uint32 counts
    (hhsr_white_balance_hist).  uint16 [H, W] sensor counts, or with `packing` (a name of utils_dng.PACKINGS) uint8
    [H, row_bytes] packed rows of `width` pixels (may be left out when the rows hold no padding), H and W even — read as
    they lie in memory, never normalised or copied.  Rows may be strided (one row stride for all frames, elements of a row
    adjacent).  `black_levels`: per colour (R, G, B).  The library is called in chunks of MAX_BATCH frames and the chunks'
    counts are added."""
    frames = list(frames)
    if not frames:
        raise ValueError("white_balance_histogram: no frame")
    f0 = frames[0]
    for t in frames:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("white_balance_histogram expects tensors on the GPU (the HIP path has no CPU fallback)")
        if t.dim() != 2 or t.shape != f0.shape or t.dtype != f0.dtype or t.device != f0.device or t.stride() != f0.stride():
            raise ValueError("white_balance_histogram: the frames need one 2-D shape, dtype, device and row stride")
    if f0.stride(1) != 1 and f0.shape[1] > 1:
        raise ValueError("white_balance_histogram: the elements of a row must be adjacent in memory")
    if cfa_pattern is None:
        raise ValueError("white_balance_histogram: a CFA pattern is required (a monochrome sensor has no white balance)")
    H, row_bytes = f0.shape[0], f0.stride(0) * f0.element_size()
    if packing is not None:
        from .utils_dng import _packing, infer_width

        if f0.dtype != torch.uint8:
            raise TypeError(f"white_balance_histogram: packed frames are uint8 [H, row_bytes] (got {f0.dtype})")
        fmt = _packing(packing)[0]
        W = infer_width(f0.shape[1], packing) if width is None else int(width)
        if W is None:
            raise ValueError("white_balance_histogram: give 'width' (the rows are longer than their pixels' bytes)")
    elif f0.dtype in (torch.uint16, torch.int16):
        fmt, W = -1, f0.shape[1]
    else:
        raise TypeError(f"white_balance_histogram: uint16 or packed uint8 sensor counts (got {f0.dtype}): normalised float "
                        "frames are already white-balanced")
    bl = [float(v) for v in list(black_levels)[:3]]
    if len(bl) < 3:
        raise ValueError("black_levels needs one entry per colour (R, G, B)")
    cfa, bl = _lib.cfa_bytes(np.asarray(cfa_pattern).tolist()), _lib.doubles(bl)
    dev = f0.device
    total = None
    with torch.cuda.device(dev):
        for i in range(0, len(frames), _lib.MAX_BATCH):
            chunk = frames[i:i + _lib.MAX_BATCH]
            hist = torch.empty(HIST_SHAPE, dtype=torch.int32, device=dev)
            _lib.call("hhsr_white_balance_hist", _lib.ptr_array(chunk), len(chunk), H, W, row_bytes, fmt, cfa, bl,
                      float(white_level), _lib.ptr(hist), _lib.stream(dev))
            total = hist if total is None else total.add_(hist)
    return total


def fit_white_balance(hist, min_tiles=MIN_TILES):
    """The fit of the library (hhsr_white_balance_fit, host code: the one implementation) on a histogram [192, 192] (device
    or host tensor, or ndarray) -> {"white_balance": [r, 1.0, b], "tiles": N, "tiles_gated": n}.  ValueError when the
    histogram holds fewer than min_tiles tiles."""
    h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    if h.size != BINS * BINS or h.dtype.kind not in "iu":
        raise ValueError(f"fit_white_balance: an integer histogram of shape {HIST_SHAPE}")
    h = np.ascontiguousarray(h.astype(np.uint32))  # (the int32 tensor of white_balance_histogram holds the uint32 bits)
    if isinstance(min_tiles, bool) or int(min_tiles) < 1:
        raise ValueError(f"fit_white_balance: min_tiles {min_tiles!r}: an integer >= 1")
    wb, tiles = (C.c_double * 3)(), (C.c_int64 * 2)()
    lib = _lib.load()
    rc = lib.hhsr_white_balance_fit(h.ctypes.data_as(C.c_void_p), int(min_tiles), wb, tiles)
    if rc == -3:
        raise ValueError(f"white balance: {int(tiles[0])} usable tiles, fewer than min_tiles = {int(min_tiles)} (frames too "
                         "small, black or clipped: measure more frames with white_balance.frames, lower "
                         "white_balance.min_tiles, or give the gains in the burst's white_balance)")
    if rc != 0:
        raise RuntimeError(f"hhsr_white_balance_fit failed (code {rc}): {lib.hhsr_last_error().decode()}")
    return {"white_balance": [float(wb[0]), float(wb[1]), float(wb[2])], "tiles": int(tiles[0]), "tiles_gated": int(tiles[1])}


def estimate_white_balance(frames, cfa_pattern, black_levels, white_level, packing=None, width=None, min_tiles=MIN_TILES):
    """The gains of integer sensor counts (one frame [H, W], a stack [n, H, W] or a list; uint16 counts or, with `packing`,
    packed uint8 rows; host data is uploaded as it is) -> the dict of fit_white_balance.  One pass over the frames on the
    GPU, 144 KiB back to the host, one host synchronisation."""
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = [frames] if frames.ndim == 2 else [frames[i] for i in range(frames.shape[0])]
    dev = None
    for f in frames:
        if torch.is_tensor(f) and f.is_cuda:
            dev = f.device
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    hist = white_balance_histogram([device_counts(f, dev, packing) for f in frames], cfa_pattern, black_levels,
                                   white_level, packing, width)
    return fit_white_balance(hist, min_tiles)


def device_counts(frame, device, packing=None):
    """One frame of integer counts on `device` in its own form: packed uint8 rows stay uint8, any other integer array becomes
    uint16 (ValueError outside its range); TypeError for float data."""
    if torch.is_tensor(frame):
        if frame.dtype.is_floating_point:
            raise TypeError("white balance: integer sensor counts expected: float frames are already white-balanced")
        return frame.to(device, non_blocking=True)
    a = np.asarray(frame)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError("white balance: integer sensor counts expected: float frames are already white-balanced")
    if packing is None and a.dtype != np.uint16:
        if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
            raise ValueError("sensor counts outside the uint16 range")
        a = a.astype(np.uint16)
    return torch.as_tensor(np.ascontiguousarray(a)).to(device, non_blocking=True)
