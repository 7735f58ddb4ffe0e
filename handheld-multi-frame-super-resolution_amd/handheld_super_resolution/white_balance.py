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
from .config import estimate_options
from .raw_frames import COUNTS, PACKED, check_device_frames, frame_list, summed_histogram, upload_frame

BINS = 192  # HHSR_WB_BINS
HIST_SHAPE = (BINS, BINS)
MIN_TILES = 16


def wb_options(config):
    """(source, frames, min_tiles) of the optional section config.white_balance = {"source": "given" | "estimate",
    "frames": 1, "min_tiles": 16} (not in the reference schema, like config.reference and config.output; absent:
    ("given", 1, 16)).  frames: how many frames of the burst, from the reference frame on, are measured.  ValueError for
    anything else."""
    return estimate_options("white_balance", config.get("white_balance", None) or {}, MIN_TILES)


def white_balance_histogram(frames, cfa_pattern, black_levels, white_level, packing=None, width=None):
    """Tile histogram of a list of device frames of one shape -> device int32 tensor [192, 192] holding the uint32 counts
    (hhsr_white_balance_hist).  uint16 [H, W] sensor counts, or with `packing` (a name of utils_dng.PACKINGS) uint8
    [H, row_bytes] packed rows of `width` pixels (may be left out when the rows hold no padding), H and W even — read as
    they lie in memory, never normalised or copied; rows may be strided (raw_frames.check_device_frames).  `black_levels`:
    per colour (R, G, B).  One call per chunk of frames (raw_frames.summed_histogram)."""
    frames = list(frames)
    H, W, row_bytes, fmt = check_device_frames("white_balance_histogram", frames, (COUNTS, PACKED), packing, width)
    if cfa_pattern is None:
        raise ValueError("white_balance_histogram: a CFA pattern is required (a monochrome sensor has no white balance)")
    bl = [float(v) for v in list(black_levels)[:3]]
    if len(bl) < 3:
        raise ValueError("black_levels needs one entry per colour (R, G, B)")
    cfa, bl = _lib.cfa_bytes(np.asarray(cfa_pattern).tolist()), _lib.doubles(bl)
    return summed_histogram(frames, HIST_SHAPE, lambda chunk, hist: _lib.call(
        "hhsr_white_balance_hist", _lib.ptr_array(chunk), len(chunk), H, W, row_bytes, fmt, cfa, bl, float(white_level),
        _lib.ptr(hist), _lib.stream(hist.device)))


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
    frames, dev = frame_list(frames)
    hist = white_balance_histogram([device_counts(f, dev, packing) for f in frames], cfa_pattern, black_levels,
                                   white_level, packing, width)
    return fit_white_balance(hist, min_tiles)


def device_counts(frame, device, packing=None):
    """One frame of integer counts on `device` in its own form (raw_frames.upload_frame); TypeError for float data."""
    return upload_frame(frame, device, packing is not None, counts_only=True)
