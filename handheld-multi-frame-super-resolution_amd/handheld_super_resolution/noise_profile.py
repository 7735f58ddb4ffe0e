"""Noise profile (alpha, beta) of a burst that brings none: variance = alpha x + beta on normalised raw values, estimated
from the frames themselves.  The reference reads the pair from the DNG NoiseProfile tag (super_resolution.py:232-238);
arrays, .npz files, sensor counts and packed rows have no such tag.

The statistic is one pass over frames in HBM (hhsr_noise_profile_hist): per 8 x 8 quad tile of one CFA plane the mean and
the energy of a 4-neighbour residual, binned into an integer histogram [4][64][1024].  The fit is host code of the same
library (hhsr_noise_profile_fit): per colour and mean bin the median energy, then a weighted line.  include/hhsr.h states
both, tests/noise_profile_ref.py is their NumPy form.

Known bias, not corrected: the median of a tile energy lies 1 - 2 % below the variance, and texture finer than a tile
counts as noise — on a textured scene the result is an upper bound."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .config import estimate_options
from .raw_frames import FLOAT, check_device_frames, frame_list, summed_histogram

HIST_SHAPE = (4, 64, 1024)
COLOURS = ("red", "green", "blue")
MIN_TILES = 16


def noise_options(config):
    """(source, frames, min_tiles) of config.noise_model: the optional keys source = "given" | "estimate" (absent: "given"),
    frames (default 1: how many frames of the burst, from the reference frame on, are measured) and min_tiles (default 16).
    ValueError for anything else, and for "estimate" together with a config.noise_model.alpha that is not None: the
    caller gave a profile and asked for another."""
    nm = config.noise_model
    source, frames, min_tiles = estimate_options("noise_model", nm, MIN_TILES)
    if source == "estimate" and nm.get("alpha", None) is not None:
        raise ValueError("config.noise_model.source 'estimate' contradicts config.noise_model.alpha = "
                         f"{nm.get('alpha')!r}: leave alpha / beta None, or set source: given")
    return source, frames, min_tiles


def inv_gains(cfa_pattern, white_balance):
    """float32 [4], one entry per CFA position: the float32 reciprocal of wb[c] / wb[1]; all 1 without a CFA."""
    if cfa_pattern is None:
        return np.ones(4, np.float32)
    if white_balance is None:
        white_balance = (1.0, 1.0, 1.0)
    wb = np.asarray([float(v) for v in list(white_balance)[:3]], np.float64)
    flat = [int(v) for v in np.asarray(cfa_pattern).reshape(-1)]
    if len(flat) != 4 or min(flat) < 0 or max(flat) > 2:
        raise ValueError(f"CFA pattern must be 2x2 with entries 0..2, got {cfa_pattern}")
    return np.array([np.float32(1.0) / np.float32(wb[c] / wb[1]) for c in flat], np.float32)


def noise_histogram(frames, cfa_pattern=None, white_balance=None):
    """Tile histogram of a list of device frames of one shape -> device int32 tensor [4, 64, 1024] holding the uint32
    counts (hhsr_noise_profile_hist).  float32 [H, W], normalised and white-balanced, H and W even; rows may be strided
    (raw_frames.check_device_frames).  `cfa_pattern` None: a monochrome sensor.  One call per chunk (summed_histogram)."""
    frames = list(frames)
    H, W, row_bytes, _ = check_device_frames("noise_histogram", frames, (FLOAT,))
    cfa = None if cfa_pattern is None else _lib.cfa_bytes(cfa_pattern)
    gains = _lib.floats(inv_gains(cfa_pattern, white_balance))
    return summed_histogram(frames, HIST_SHAPE, lambda chunk, hist: _lib.call(
        "hhsr_noise_profile_hist", _lib.ptr_array(chunk), len(chunk), H, W, row_bytes, cfa, gains, _lib.ptr(hist),
        _lib.stream(hist.device)))


def fit_profile(hist, cfa_pattern=None, min_tiles=MIN_TILES):
    """The line fit of the library (hhsr_noise_profile_fit, host code: the one implementation) on a histogram
    [4, 64, 1024] (device or host tensor, or ndarray) -> {"alpha", "beta": the mean over the colours, "per_colour":
    [(alpha, beta)] for R, G, B, "bins_used": [3]}.  ValueError when a colour has fewer than 2 usable mean bins."""
    h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    if h.size != int(np.prod(HIST_SHAPE)) or h.dtype.kind not in "iu":
        raise ValueError(f"fit_profile: an integer histogram of shape {HIST_SHAPE}")
    h = np.ascontiguousarray(h.astype(np.uint32))  # (the int32 tensor of noise_histogram holds the uint32 bits)
    if isinstance(min_tiles, bool) or int(min_tiles) < 1:
        raise ValueError(f"fit_profile: min_tiles {min_tiles!r}: an integer >= 1")
    cfa = None if cfa_pattern is None else _lib.cfa_bytes(cfa_pattern)
    ab, used = (C.c_double * 8)(), (C.c_int32 * 3)()
    lib = _lib.load()
    rc = lib.hhsr_noise_profile_fit(h.ctypes.data_as(C.c_void_p), cfa, int(min_tiles), ab, used)
    if rc == -3:
        bad = [c for c in range(3) if used[c] < 2]
        what = "the frame" if cfa is None else COLOURS[bad[0]]
        raise ValueError(f"noise profile: {what} has {used[bad[0]]} usable mean bins of at least {int(min_tiles)} tiles, a "
                         "line needs 2 (frames too small, clipped or of one brightness: measure more frames, lower "
                         "noise_model.min_tiles, or give alpha / beta)")
    if rc != 0:
        raise RuntimeError(f"hhsr_noise_profile_fit failed (code {rc}): {lib.hhsr_last_error().decode()}")
    return {"alpha": float(ab[6]), "beta": float(ab[7]),
            "per_colour": [(float(ab[2 * c]), float(ab[2 * c + 1])) for c in range(3)],
            "bins_used": [int(used[c]) for c in range(3)]}


def estimate_noise_profile(frames, cfa_pattern=None, white_balance=None, min_tiles=MIN_TILES):
    """(alpha, beta) of normalised, white-balanced float32 frames (one frame [H, W], a stack [n, H, W] or a list; host data
    is uploaded) -> the dict of fit_profile.  One pass over the frames on the GPU, 1 MiB back to the host, one host
    synchronisation."""
    frames, dev = frame_list(frames)
    dev_frames = [_lib.f32c(f, dev) for f in frames]
    return fit_profile(noise_histogram(dev_frames, cfa_pattern, white_balance), cfa_pattern, min_tiles)
